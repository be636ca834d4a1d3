// cells_verify_async.hip -- lwkzg_cell_verifier_*: lwkzg_verify_cell_kzg_proof_batch_device without a parked host thread (DESIGN.md
// section 4n), the counterpart of verify_async.hip for cells.
//
// The synchronous call stops its thread three times and works on the host in between: the commitments and indices come down to be
// grouped (cells_verify_api.hip: group_items), the digests come down to be hashed into r, the sums come down for the pairing. Here the
// grouping is kernels (cell_group.hip), both remaining pieces of host work are HOST FUNCTIONS in stream order, and the verdict lands in
// a LwkzgCellVerifyResult whose state word is stored last:
//
//   caller's stream --event--> context stream: grouping, digests, two-set validation, fault words
//                              head (m, bad index, error), fault words, first_item, digests, padded commitments -> pinned
//                                                                                |  side stream: k_vmsm_multiples (both point sets)
//                              HOST FUNCTION 1: first_bad and the code, or r and its 33 powers; the skip word -> pinned
//                              powers + skip word -> device
//                              k_cellv_scalars, row weights (n workgroups, m from memory), columns, coefficients, the 64-term MSM on
//                              the engine's launch set, k_vmsm_accumulate / bucket sums / weighted; 348 bytes -> pinned
//                              HOST FUNCTION 2: cell_batch_finish (the pairing), the result, state = 1 (release), slot freed
//   caller's stream <--event-- (work enqueued behind the call sees the verdict)
//
// Calls on one verifier share its device block and pinned block and run one after the other: on one context by stream order, across
// the settings' two contexts (pick_ctx) by the verifier's last_done event. The job slots and the protocol of a failing enqueue are
// verifier_ring.h; the handle's head, the enqueue around enqueue_on, pending / wait / free and the host functions' rules are
// async_verifier.h, shared with verify_async.hip. What the host functions DECIDE -- the first fault, the code or r, a grouped call's
// two steps -- is cells_verify_host.h and the first visit cells_verify.hip's launch_cellv_first_visit, both shared with the synchronous
// grouped call (cells_verify_groups.hip); this file keeps the host functions themselves, the enqueue code and the *_host_steps hooks.
//
// A verifier made by lwkzg_cell_verifier_new_groups also takes GROUPED calls (lwkzg_cell_verifier_enqueue_groups):
// lwkzg_verify_cell_kzg_proof_groups_device's answers, one per group, through the same shell -- the segmented grouping and the slice
// table of cell_group.hip, the launches and the buffers behind r of cells_verify_groups.h (CellgBufs, CellgPin), two host functions
// of their own around groups_decide and groups_answers (enqueue_groups_on below).
//
// A verifier made by lwkzg_cell_verifier_new_blobs also takes WHOLE BLOBS (lwkzg_cell_verifier_enqueue_blobs / _blobs_groups; DESIGN.md
// section 4t): the answers of lwkzg_verify_blob_cell_kzg_proofs_batch_device / _groups_device through the same two enqueue functions.
// Where a call's items and lists come from is their parameter (CallItems): the caller's four arrays and the item-level grouping, or
// blob_items_on -- the blobs extended into the verifier's scratch (cells_verify_blobs.h: launch_blob_cells), their n commitments
// grouped by one workgroup and every 128 n-entry list written from its tables (cell_blobs_group.hip) -- and, behind the first visit,
// the rejected blobs' status words folded into the fault words. Nothing of a blob call comes down but what the host functions read.
#include "abi_guard.h"
#include "async_verifier.h"
#include "cell_blobs_group.h"
#include "cell_group.cuh"
#include "cells_verify_blobs.h"
#include "cells_verify_groups.h"
#include "cells_verify_host.h"
#include "cellv_bufs.h"

#include <chrono>
#include <new>
#include <random>
#include <vector>

namespace lwk {

namespace {

constexpr uint64_t kCellVerifierMagic = 0x4c574b5a43564659ull;  // "LWKZCVFY"
constexpr size_t kPinPowers = 33 * sizeof(Fr) + 4;   // the powers and, behind them, the skip word: one copy up
constexpr size_t kPinSums = 3 * 96 + 3 * 4 + 48;     // the three sums, their flags, RLI: 348 bytes down

// what a GROUPED call keeps beside its job slot (section 4r): where its answers go, and its own copy of the offsets
struct GroupCall {
    uint8_t *ok_out = nullptr, *partials_out = nullptr;
    int32_t *rc_out = nullptr;
    size_t g = 0;
    uint32_t *h_off = nullptr;   // pinned, gcap + 1 words of this slot alone: the upload reads it after the enqueue has returned
};

static_assert(kBlobGroupCap == kCellsChunk, "a blob call is one extension chunk, grouped by one workgroup");

// what a BLOB call reads its items from (section 4t); the verifier's own, out of its device block
struct BlobScratch {
    uint8_t *cells = nullptr;      // 256 KiB per blob: the 128 cells the extension leaves
    uint64_t *idx = nullptr;       // the expanded items' indices
    int32_t *status = nullptr;     // one word per blob: the extension's verdict
    BlobGroupOut tab = {};         // the per-blob tables of the grouping (cell_blobs_group.h); distinct and head are the call's
};

// where a call's items and lists come from: the caller's four arrays (an item call), or nb whole blobs (blobs != nullptr), whose
// cells and indices blob_items_on leaves in the verifier's scratch
struct CallItems {
    const uint8_t *comms, *cells, *proofs;
    const uint64_t *idx;
    const uint8_t *blobs = nullptr;
    size_t nb = 0;
};

struct CellVerifier : AsyncVerifier {
    // ---- blob calls (lwkzg_cell_verifier_new_blobs; bcap == 0: none) ----
    size_t bcap = 0;
    BlobScratch bs;
    // ---- grouped calls (lwkzg_cell_verifier_new_groups; gcap == 0: none) ----
    size_t gcap = 0, max_slices = 0;
    CellGroupSegBufs sg;
    CellgBufs gb = {};                // behind r (cells_verify_groups.h)
    CellgPin gp = {};
    uint32_t *h_rowbase = nullptr, *h_gbad = nullptr, *h_offs = nullptr;
    GroupCall gcall[LWKZG_VERIFIER_DEPTH];
    // between the two host functions of ONE call (calls of a verifier run one after the other): every group's code and r
    std::vector<int32_t> g_rc;
    std::vector<uint32_t> g_r;
    // ---- every call ----
    size_t slots = 0;
    uint64_t seed = 0;                // of the slot hash, drawn once
    uint8_t *dev = nullptr;           // one block: CellvBufs, the grouping's scratch, the fault words
    CellvBufs b;
    CellGroupBufs g;
    int32_t *fault = nullptr;         // 2 cap words (k_cellv_fault_words)
    uint8_t *pin = nullptr;           // hipHostMalloc, carved below
    uint32_t *h_head = nullptr, *h_first = nullptr;
    int32_t *h_fault = nullptr;
    uint8_t *h_dig = nullptr, *h_comm = nullptr, *h_up = nullptr, *h_sums = nullptr;
    hipEvent_t ev_in = nullptr, ev_fork = nullptr, ev_rows = nullptr;
    // g2_values[0] and g2_values[64] of the settings, copied at creation: all the host functions ever see of them
    g2_t g2[65];
    KZGSettings own;
    CellVerifier(Ctx *c, const KZGSettings *s, size_t max_cells) : AsyncVerifier(kCellVerifierMagic, c, s, max_cells) {}
    void free_own() {
        if (dev) (void)hipFree(dev);
        if (pin) (void)hipHostFree(pin);
        for (hipEvent_t e : {ev_in, ev_fork, ev_rows})
            if (e) (void)hipEventDestroy(e);
    }
};

size_t carve_device(CellVerifier *v, uint8_t *base) {
    Carver cv(base);
    cellv_carve(v->b, cv, v->cap, false);
    cell_group_carve(v->g, cv, v->cap, v->slots);
    cv.take(v->fault, 2 * v->cap * 4);
    v->g.rows = v->b.rows;
    v->g.perm_row = v->b.perm_row;
    v->g.row_off = v->b.row_off;
    v->g.perm_col = v->b.perm_col;
    v->g.col_off = v->b.col_off;
    v->g.distinct = v->b.comm_in;
    if (v->gcap) {
        const size_t gc = v->gcap;
        cell_group_seg_carve(v->sg, v->g, cv, v->cap, gc);
        cellg_carve(v->gb, cv, gc, v->max_slices);
    }
    if (v->bcap) {
        const size_t nb = v->bcap;
        BlobScratch &s = v->bs;
        cv.take(s.cells, nb * kBlobCellBytes);
        cv.take(s.idx, nb * kCellsPerBlob * 8);
        cv.take(s.status, nb * 4);
        cv.take(s.tab.brow, nb * 4);
        cv.take(s.tab.bgroup, nb * 4);
        cv.take(s.tab.bperm, nb * 4);
        cv.take(s.tab.brow_off, (nb + 1) * 4);
        cv.take(s.tab.bfirst, nb * 4);
    }
    return cv.bytes();
}

size_t carve_pinned(CellVerifier *v, uint8_t *base) {
    Carver cv(base);
    cv.take(v->h_head, kGroupHeadWords * 4);
    cv.take(v->h_fault, 2 * v->cap * 4);
    cv.take(v->h_first, v->cap * 4);
    cv.take(v->h_dig, v->cap * 32);
    cv.take(v->h_comm, v->cap * 48);
    cv.take(v->h_up, kPinPowers);
    cv.take(v->h_sums, kPinSums);
    if (v->gcap) {
        const size_t gc = v->gcap;
        cv.take(v->h_rowbase, (gc + 1) * 4);
        cv.take(v->h_gbad, gc * 4);
        cellg_carve_pin(v->gp, cv, gc);
        cv.take(v->h_offs, LWKZG_VERIFIER_DEPTH * (gc + 1) * 4);
        for (int k = 0; k < LWKZG_VERIFIER_DEPTH; k++) v->gcall[k].h_off = v->h_offs + (size_t)k * (gc + 1);
    }
    return cv.bytes();
}

// ---- the two host functions ------------------------------------------------------------------------------------------------------
// Their rules are async_verifier.h's. What they call keeps to them: cell_batch_challenge and cell_batch_powers hash and multiply;
// cell_batch_finish's pairing takes fixed_q_lines' cache mutex (pairing.hip), which guards a search and a push_back and is never held
// across a wait for the GPU or across the lines' computation; its two set_error calls (a NULL g2_values, an interpolant's commitment
// that is no point) cannot happen with a verifier's own copy of the G2 points and the engine's own compressed output, and would only
// write the runtime thread's own error text.

// behind the copies of the head, the fault words, the digests and the padded commitments: decide_or_challenge (cells_verify_host.h)
void cell_verifier_host_fn1(void *p) {
    AsyncJob *j = (AsyncJob *)p;
    CellVerifier *v = static_cast<CellVerifier *>(j->v);
    uint32_t skip = 1;
    try {
        const uint32_t m = v->h_head[kGroupHeadM], bad_index = ~v->h_head[kGroupHeadBad];
        j->m = m;
        if (v->h_head[kGroupHeadErr] != 0 || m == 0 || m > j->n) {
            j->failed = true;
        } else {
            uint32_t r_raw[8];
            if (decide_or_challenge(r_raw, &j->first_bad, &j->code, v->h_comm, m, v->h_dig, j->n, bad_index, v->h_fault, v->h_fault + j->n, v->h_first,
                                    j->mode)) {
                cell_batch_powers((Fr *)v->h_up, r_raw);
                cell_r_bytes(((LwkzgCellVerifyResult *)j->res)->partials, r_raw, j->mode);
                skip = 0;
            }
        }
    } catch (...) {
        j->failed = true;
    }
    memcpy(v->h_up + 33 * sizeof(Fr), &skip, 4);
}

// behind the copy of the three sums and RLI: the pairing, the partials, the state word last, the slot freed
void cell_verifier_host_fn2(void *p) {
    AsyncJob *j = (AsyncJob *)p;
    CellVerifier *v = static_cast<CellVerifier *>(j->v);
    LwkzgCellVerifyResult *res = (LwkzgCellVerifyResult *)j->res;
    C_KZG_RET rc = C_KZG_ERROR;
    bool ok = false;
    try {
        if (j->failed) {
            rc = C_KZG_ERROR;
        } else if (j->first_bad != kNoneBad) {
            rc = (C_KZG_RET)j->code;
        } else {
            uint8_t sums[3][96], rli48[48];
            int infs[3];
            sums_from_pinned(sums, infs, v->h_sums, v->h_sums + 3 * 96);
            memcpy(rli48, v->h_sums + 3 * 96 + 12, 48);
            rc = cell_batch_finish(&ok, res->partials + 32, sums, infs, rli48, &v->own);
        }
    } catch (...) {
        rc = C_KZG_ERROR;
    }
    if (rc != C_KZG_OK) memset(res->partials, 0, sizeof res->partials);
    res->first_bad = j->first_bad;
    res->m = j->m;
    complete_now(res, rc, ok && rc == C_KZG_OK);
    v->ring.release(j);   // (the verifier may be gone as soon as this returns)
}

// ---- a grouped call's result, behind its two host steps (cells_verify_host.h: groups_decide, groups_answers) ----------------------------------
// The groups' answers and partials, then the result's fields, then state. failed: step 1 could not do its work
template <class SumsOf>
void groups_finish(LwkzgCellVerifyResult *res, uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out, int32_t *rc, const uint32_t *r_raw,
                   const uint32_t *flags, const uint32_t *off, size_t g, uint32_t m_total, const KZGSettings *own, int mode, bool failed,
                   const SumsOf &sums_of) {
    if (failed) {
        if (partials_out) memset(partials_out, 0, g * (size_t)LWKZG_CELL_VERIFY_PARTIAL_BYTES);
        for (size_t j = 0; j < g; j++) rc_out[j] = (int32_t)C_KZG_ERROR, ok_out[j] = 0;
    } else {
        groups_answers(ok_out, rc_out, partials_out, rc, r_raw, flags, off, g, own, mode, sums_of);
    }
    uint32_t first_bad = kNoneBad;
    for (size_t j = 0; j < g && first_bad == kNoneBad; j++)
        if (rc_out[j] != (int32_t)C_KZG_OK || ok_out[j] != 1) first_bad = (uint32_t)j;
    res->first_bad = first_bad;
    res->m = m_total;
    complete_now(res, failed ? C_KZG_ERROR : C_KZG_OK, !failed && first_bad == kNoneBad);
}

// ---- the two host functions of a grouped call (rules: async_verifier.h; host_parallel_for's pool is taken in turns and no job of it
// ever waits for the GPU) ----
// behind the copies of the head, row_base, the bad words, the fault words, first_item, the digests and the concatenated commitments
void cell_verifier_groups_fn1(void *p) {
    AsyncJob *j = (AsyncJob *)p;
    CellVerifier *v = static_cast<CellVerifier *>(j->v);
    const GroupCall &gc = v->gcall[j - v->ring.slots];
    uint32_t *flags = v->gp.gflag(gc.g);
    try {
        const uint32_t m = v->h_head[kGroupHeadM];
        j->m = m;
        if (v->h_head[kGroupHeadErr] != 0 || m > j->n || v->h_rowbase[gc.g] != m) j->failed = true;
        else
            groups_decide(v->g_rc.data(), v->g_r.data(), v->gp.pw(), flags, gc.h_off, gc.g, j->n, v->h_rowbase, v->h_gbad, v->h_fault,
                          v->h_first, v->h_dig, v->h_comm, j->mode);
    } catch (...) {
        j->failed = true;
    }
    if (j->failed)
        for (size_t k = 0; k < gc.g; k++) flags[k] = 1;
}

// behind the copies of the sums, their flags and the RLIs
void cell_verifier_groups_fn2(void *p) {
    AsyncJob *j = (AsyncJob *)p;
    CellVerifier *v = static_cast<CellVerifier *>(j->v);
    const GroupCall &gc = v->gcall[j - v->ring.slots];
    LwkzgCellVerifyResult *res = (LwkzgCellVerifyResult *)j->res;
    const uint32_t *flags = v->gp.gflag(gc.g);
    bool failed = j->failed;
    try {
        groups_finish(res, gc.ok_out, gc.rc_out, gc.partials_out, v->g_rc.data(), v->g_r.data(), flags, gc.h_off, gc.g, j->m, &v->own, j->mode,
                      failed, [&](size_t k, uint8_t sums[3][96], int infs[3], uint8_t rli48[48]) {
                          sums_from_pinned(sums, infs, v->gp.sums + 3 * 96 * k, (const uint8_t *)(v->gp.inf + 3 * k));
                          memcpy(rli48, v->gp.rli48 + 48 * k, 48);
                          return true;
                      });
    } catch (...) {   // (the pool could not take the job: nothing of the result is final yet)
        res->first_bad = 0;
        complete_now(res, C_KZG_ERROR, false);
    }
    v->ring.release(j);   // (the verifier may be gone as soon as this returns)
}

// the workspace a call on context c takes: one MSM slot, or a grouped call's launch set
C_KZG_RET reserve_for(Ctx *c, size_t msm_slots) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    C_KZG_RET rc = ctx_reserve(c, msm_slots);
    if (rc != C_KZG_OK) return rc;
    stream_warm_host_fn(c->stream);
    return C_KZG_OK;
}

uint64_t draw_seed(const void *salt) {
    uint64_t s = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() ^ (uint64_t)(uintptr_t)salt;
    try {
        std::random_device rd;
        s ^= ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    } catch (...) {   // no entropy source: the clock and the address it is
    }
    return s;
}

// max_groups == 0: a verifier of batch calls alone (lwkzg_cell_verifier_new); max_blobs > 0: max_cells is 128 max_blobs and the verifier
// takes blob calls too (lwkzg_cell_verifier_new_blobs)
C_KZG_RET cell_verifier_new_impl(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_cells, size_t max_groups, size_t max_blobs = 0) {
    if (!out) return C_KZG_BADARGS;
    *out = nullptr;
    if (!s || max_cells == 0 || max_cells >= 0x40000000u || max_groups > 0x40000000u) return C_KZG_BADARGS;
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (!s->g2_values) {
        set_error("lwkzg_cell_verifier_new: the settings have no g2_values");
        return C_KZG_BADARGS;
    }
    ensure_lagrange(c, mode_of(s));
    CellVerifier *v = new (std::nothrow) CellVerifier(c, s, max_cells);
    if (!v) return C_KZG_MALLOC;
    v->slots = group_table_slots(max_cells);
    v->gcap = max_groups;
    v->bcap = max_blobs;
    v->max_slices = max_groups ? plan_max_slices(max_cells, max_groups) : 0;
    v->seed = draw_seed(v);
    memset(v->g2, 0, sizeof v->g2);
    v->g2[0] = s->g2_values[0];
    v->g2[64] = s->g2_values[64];
    v->own.fs = nullptr;
    v->own.g1_values = nullptr;
    v->own.g2_values = v->g2;
    // a blob call's extension takes what cells_chunks reserves for a chunk without proofs: two slots per blob
    const size_t group_slots = max_groups ? min_sz(max_groups, kMaxChunk) : 1, msm_slots = group_slots > 2 * max_blobs ? group_slots : 2 * max_blobs;
    C_KZG_RET rc = C_KZG_OK;
    try {
        v->g_rc.resize(max_groups);
        v->g_r.resize(8 * max_groups);
    } catch (...) {
        rc = C_KZG_MALLOC;
    }
    if (rc == C_KZG_OK) rc = reserve_for(c, msm_slots);
    if (rc == C_KZG_OK)
        if (Ctx *t = c->twin.load(std::memory_order_acquire)) rc = reserve_for(t, msm_slots);
    if (rc == C_KZG_OK) {
        std::lock_guard<std::mutex> lk(c->mu);
        const size_t dev_bytes = carve_device(v, nullptr), pin_bytes = carve_pinned(v, nullptr);
        const bool ok = hipMalloc((void **)&v->dev, dev_bytes) == hipSuccess && hipHostMalloc((void **)&v->pin, pin_bytes, hipHostMallocDefault) == hipSuccess &&
                        hipEventCreateWithFlags(&v->ev_in, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&v->ev_fork, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&v->ev_rows, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&v->last_done, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            set_error("lwkzg_cell_verifier_new: no memory or events for %zu cells (%zu bytes on the device, %zu pinned)", max_cells, dev_bytes,
                      pin_bytes);
            rc = C_KZG_MALLOC;
        } else {
            carve_device(v, v->dev);
            carve_pinned(v, v->pin);
        }
    }
    return async_verifier_new_end(out, v, rc);
}

// ---- the items of a blob call -----------------------------------------------------------------------------------------
// On st, in front of the first visit, for the it.nb blobs of the call: the extension into the verifier's scratch with a status word per
// blob; the commitments grouped (k_blob_group, one workgroup); every list of the 128 nb items where the pipeline reads it
// (k_blob_items_dev). g == 0: a batch call -- the lists of v->g, one group of all blobs; else a grouped call of g groups -- the lists
// of v->sg, whose item_off the caller has uploaded (in items), and zero bad words. Leaves it.cells and it.idx at the scratch
C_KZG_RET blob_items_on(CellVerifier *v, Ctx *c, const AsyncJob *j, CallItems &it, size_t g, hipStream_t st) {
    BlobScratch &s = v->bs;
    const CellGroupSegBufs &sg = v->sg;
    C_KZG_RET rc = launch_blob_cells(c, s.cells, s.status, it.blobs, it.nb, j->mode, st);
    if (rc != C_KZG_OK) return rc;
    BlobGroupOut tab = s.tab;
    tab.row_base = g ? sg.row_base : nullptr;
    tab.distinct = v->b.comm_in;   // (v->g.distinct and v->sg.distinct)
    tab.head = g ? sg.head : v->g.head;
    const uint32_t *item_off = g ? sg.item_off : nullptr;
    if (g) LWK_HIP(hipMemsetAsync(sg.gbad, 0, g * 4, st));
    LWK_HIP(launch_cell_blobs_group(it.comms, item_off, it.nb, g ? g : 1, v->seed, 0xffffffffu, tab, st));
    const BlobItemsOut lists{s.idx, v->b.rows, v->b.perm_row, v->b.perm_col, g ? sg.item_group : nullptr, g ? sg.col_off : v->b.col_off,
                             v->b.row_off, v->g.first_item};   // (the lists of v->g and v->sg are v->b's)
    LWK_HIP(launch_cell_blobs_items(tab, item_off, it.nb, g ? g : 1, lists, st));
    it.cells = s.cells;
    it.idx = s.idx;
    return C_KZG_OK;
}

// everything of one call on context c, enqueued; caller holds c->mu. *hf: host functions handed to the runtime so far
C_KZG_RET enqueue_on(CellVerifier *v, Ctx *c, AsyncJob *j, CallItems it, hipStream_t caller, int *hf) {
    LWK_HIP(hipSetDevice(c->device));
    C_KZG_RET rc = ctx_reserve(c, 1);   // (at once unless this context was made after the verifier)
    if (rc != C_KZG_OK) return rc;
    CellvBufs &b = v->b;
    const size_t n = j->n;
    const int le = mode_rules(j->mode).le(), bad = (int)bad_input(j->mode);
    hipStream_t st = c->stream, side = c->aux[1];
    const uint32_t *d_m = v->g.head + kGroupHeadM;
    uint32_t *d_skip = (uint32_t *)(b.pw + 33);
    if ((rc = async_enqueue_head(v, c)) != C_KZG_OK) return rc;
    if (caller && caller != st) {   // the inputs were produced on the caller's stream
        LWK_HIP(hipEventRecord(v->ev_in, caller));
        LWK_HIP(hipStreamWaitEvent(st, v->ev_in, 0));
    }
    WsUse wsu(c, st);
    LWK_HIP(hipMemsetAsync(b.sc_c, 0, 32 * n, st));
    if (it.blobs) {
        if ((rc = blob_items_on(v, c, j, it, 0, st)) != C_KZG_OK) return rc;
    } else {
        launch_cell_group(it.comms, it.idx, n, v->slots, v->seed, 0xffffffffu, v->g, st);
    }
    const uint8_t *cells = it.cells, *proofs = it.proofs;
    const uint64_t *idx = it.idx;
    const PointSet set_p{proofs, b.pts_p, b.kind_p, b.canon_p, b.verdict_p}, set_c{b.comm_in, b.pts_c, b.kind_c, b.canon_c, b.verdict_c};
    LWK_HIP(launch_cellv_first_visit(cells, idx, b.rows, set_p, set_c, b.digests, v->fault, b.status, bad, le, n, st));
    if (it.blobs) LWK_HIP(launch_blob_fold_status(v->fault, v->bs.status, it.nb, j->mode, bad, st));
    LWK_HIP(hipEventRecord(v->ev_fork, st));
    LWK_HIP(hipStreamWaitEvent(side, v->ev_fork, 0));
    launch_vmsm_multiples2(b.pts_p, b.kind_p, b.tab_p, b.pts_c, b.kind_c, b.tab_c, b.vm_tmp, b.vm_pre, n, side);   // beside the copies and the hash
    LWK_HIP(hipEventRecord(v->ev_rows, side));
    LWK_HIP(hipMemcpyAsync(v->h_head, v->g.head, kGroupHeadWords * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_fault, v->fault, 8 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_first, v->g.first_item, 4 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_dig, b.digests, 32 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_comm, b.comm_in, 48 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipLaunchHostFunc(st, cell_verifier_host_fn1, j));
    *hf = 1;
    LWK_HIP(hipMemcpyAsync(b.pw, v->h_up, kPinPowers, hipMemcpyHostToDevice, st));
    launch_cellv_scalars(b.pw, idx, c->tw_fwd, b.a_mont, b.sc_a, b.sc_b, b.perm_row, b.row_off, b.sc_c, n, n, st, d_m, d_skip);
    launch_cellv_interpolant(cells, b.a_mont, b.perm_col, b.col_off, c->tw_inv, b.colcoef, c->ws.scalars2, le, st, d_skip);
    const bool lg = coefficients_to_msm_form(c, j->mode, 1, st);
    msm_stages(c, c->ws.scalars2, b.rli48, 1, st, 0, false, lg);
    LWK_HIP(hipStreamWaitEvent(st, v->ev_rows, 0));
    launch_vmsm_accumulate(b.sc_a, b.sc_b, b.tab_p, b.kind_p, b.tab_c, b.kind_c, b.partial, n, st, b.sc_c, d_skip);
    launch_vmsm_reduce(b.partial, b.bsum, b.out96, b.inf, n, st, d_skip);
    LWK_HIP(hipMemcpyAsync(v->h_sums, b.out96, 3 * 96, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_sums + 3 * 96, b.inf, 3 * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_sums + 3 * 96 + 12, b.rli48, 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipGetLastError());
    LWK_HIP(hipLaunchHostFunc(st, cell_verifier_host_fn2, j));
    *hf = 2;
    return async_enqueue_tail(v, c, caller);
}

C_KZG_RET cell_verifier_enqueue_impl(const LwkzgCellVerifier *handle, LwkzgCellVerifyResult *res, const uint8_t *comms, const uint64_t *idx,
                                     const uint8_t *cells, const uint8_t *proofs, size_t n, hipStream_t caller) {
    AsyncVerifier *base;
    const C_KZG_RET refused = async_enqueue_checks(&base, handle, kCellVerifierMagic, res, n, "lwkzg_cell_verifier_enqueue", "cells");
    if (refused != C_KZG_OK) return refused;
    CellVerifier *v = static_cast<CellVerifier *>(base);
    if (n == 0) {   // the consensus specs' and c-kzg-4844 2.x's rule for cells, in both modes
        complete_now(res, C_KZG_OK, true);
        return C_KZG_OK;
    }
    if (!comms || !idx || !cells || !proofs) return async_refuse(res, C_KZG_BADARGS);
    const int mode = mode_of(v->s);
    ensure_lagrange(v->ctx, mode);   // (a load unless the mode changed to c-kzg after lwkzg_cell_verifier_new)
    std::lock_guard<std::mutex> enq(v->enq_mu);
    return async_enqueue(v, res, n, mode, caller,
                         [&](Ctx *c, AsyncJob *j, int *hf) { return enqueue_on(v, c, j, CallItems{comms, cells, proofs, idx}, caller, hf); });
}

// ---- a grouped call --------------------------------------------------------------------------------------------------
//   context stream: the offsets up; the segmented grouping (cell_group.hip); digests with the group-local rows; two-set validation over
//                   the items and the concatenated distinct commitments; fault words
//                   head, row_base, bad words, fault words, first_item, digests, concatenated commitments -> pinned
//                   HOST FUNCTION 1: per group the code, or r and its 33 powers; one flag word per group -> pinned
//                   powers + flags -> device (one copy); the slice table; k_cellg_scalars, row weights (n workgroups, M from memory),
//                   the interpolants and their MSMs a launch set at a time, k_cellg_slices on plan_max_slices(n, g) workgroups (the
//                   live count from memory), k_cellg_fold; sums, flags and RLIs -> pinned, one copy each
//                   HOST FUNCTION 2: the g pairings on the host threads -- the stream stands still for them --, the outputs, the
//                   result, state = 1 (release), slot freed
C_KZG_RET enqueue_groups_on(CellVerifier *v, Ctx *c, AsyncJob *j, CallItems it, hipStream_t caller, int *hf) {
    LWK_HIP(hipSetDevice(c->device));
    C_KZG_RET rc = ctx_reserve(c, min_sz(v->gcap, kMaxChunk));   // (at once unless this context was made after the verifier)
    if (rc != C_KZG_OK) return rc;
    CellvBufs &b = v->b;
    const CellGroupSegBufs &sg = v->sg;
    const GroupCall &gc = v->gcall[j - v->ring.slots];
    const size_t n = j->n, g = gc.g;
    const int le = mode_rules(j->mode).le(), bad = (int)bad_input(j->mode);
    hipStream_t st = c->stream;
    const CellgBufs &gb = v->gb;
    const Fr *d_pw = gb.pw();
    const uint32_t *d_gflag = gb.gflag(g);
    if ((rc = async_enqueue_head(v, c)) != C_KZG_OK) return rc;
    if (caller && caller != st) {   // the inputs were produced on the caller's stream
        LWK_HIP(hipEventRecord(v->ev_in, caller));
        LWK_HIP(hipStreamWaitEvent(st, v->ev_in, 0));
    }
    WsUse wsu(c, st);
    LWK_HIP(hipMemcpyAsync(sg.item_off, gc.h_off, (g + 1) * 4, hipMemcpyHostToDevice, st));
    if (it.blobs) {
        if ((rc = blob_items_on(v, c, j, it, g, st)) != C_KZG_OK) return rc;
    } else {
        launch_cell_group_seg(it.comms, it.idx, n, g, v->slots, v->seed, 0xffffffffu, sg, st);
    }
    const uint8_t *cells = it.cells, *proofs = it.proofs;
    const uint64_t *idx = it.idx;
    const PointSet set_p{proofs, b.pts_p, b.kind_p, b.canon_p, b.verdict_p}, set_c{b.comm_in, b.pts_c, b.kind_c, b.canon_c, b.verdict_c};
    LWK_HIP(launch_cellv_first_visit(cells, idx, sg.rows, set_p, set_c, b.digests, v->fault, b.status, bad, le, n, st));
    if (it.blobs) LWK_HIP(launch_blob_fold_status(v->fault, v->bs.status, it.nb, j->mode, bad, st));
    LWK_HIP(hipMemcpyAsync(v->h_head, sg.head, kGroupHeadWords * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_rowbase, sg.row_base, (g + 1) * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_gbad, sg.gbad, g * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_fault, v->fault, 8 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_first, sg.first_item, 4 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_dig, b.digests, 32 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->h_comm, b.comm_in, 48 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipLaunchHostFunc(st, cell_verifier_groups_fn1, j));
    *hf = 1;
    LWK_HIP(hipMemcpyAsync(gb.up, v->gp.up, g * kGroupUpBytes, hipMemcpyHostToDevice, st));
    const size_t workgroups = plan_max_slices(n, g);   // (at most v->max_slices: n and g are within the verifier's capacities)
    launch_cell_group_slice_table(sg.item_off, sg.row_base, d_gflag, gb.slices, gb.slice_off, g, workgroups, st);
    LWK_HIP(hipMemsetAsync(b.a_mont, 0, n * sizeof(Fr), st));   // (the row weights read whole rows: a flagged group's stay defined)
    launch_cellg_scalars(d_pw, idx, c->tw_fwd, sg.item_group, sg.item_off, d_gflag, b.a_mont, b.sc_a, b.sc_b, n, st);
    launch_cellv_row_weights(b.a_mont, sg.perm_row, sg.row_off, b.sc_c, n, st, sg.head + kGroupHeadM);
    launch_cellg_interpolants(c, j->mode, cells, b.a_mont, sg.perm_col, sg.col_off, d_gflag, gb.colcoef, gb.rli48, le, g, st);
    launch_cellg_sums(gb.slices, gb.slice_off, d_gflag, b.sc_a, b.sc_b, b.sc_c, b.pts_p, b.kind_p, b.pts_c, b.kind_c, gb.part, gb.out96, gb.inf,
                      workgroups, gb.slice_off + 3 * g, g, st);
    LWK_HIP(hipMemcpyAsync(v->gp.sums, gb.out96, 3 * 96 * g, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->gp.inf, gb.inf, 3 * 4 * g, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(v->gp.rli48, gb.rli48, 48 * g, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipGetLastError());
    LWK_HIP(hipLaunchHostFunc(st, cell_verifier_groups_fn2, j));
    *hf = 2;
    return async_enqueue_tail(v, c, caller);
}

C_KZG_RET cell_verifier_enqueue_groups_impl(const LwkzgCellVerifier *handle, LwkzgCellVerifyResult *res, uint8_t *ok_out, int32_t *rc_out,
                                            uint8_t *partials_out, const uint8_t *comms, const uint64_t *idx, const uint8_t *cells,
                                            const uint8_t *proofs, size_t n, const uint64_t *offsets, size_t g, hipStream_t caller) {
    const char *fn = "lwkzg_cell_verifier_enqueue_groups";
    AsyncVerifier *base;
    const C_KZG_RET refused = async_enqueue_checks(&base, handle, kCellVerifierMagic, res, n, fn, "cells");
    if (refused != C_KZG_OK) return refused;
    CellVerifier *v = static_cast<CellVerifier *>(base);
    if (v->gcap == 0 || g > v->gcap) {
        set_error(v->gcap ? "%s: %zu groups, the verifier was created for %zu" : "%s: the verifier was not created by lwkzg_cell_verifier_new_groups",
                  fn, g, v->gcap);
        return async_refuse(res, C_KZG_BADARGS);
    }
    if ((g > 0 && (!ok_out || !rc_out || !offsets)) || (n > 0 && (!comms || !idx || !cells || !proofs))) {
        set_error("%s: NULL argument", fn);
        return async_refuse(res, C_KZG_BADARGS);
    }
    if (!group_offsets_valid(offsets, g, n)) {
        set_error("%s: group_offsets must be %zu ascending values from 0 to %zu", fn, g + 1, n);
        return async_refuse(res, C_KZG_BADARGS);
    }
    if (n == 0) {   // no group, or empty groups alone: the batch call's answer to n == 0 for each
        for (size_t j = 0; j < g; j++) rc_out[j] = (int32_t)C_KZG_OK, ok_out[j] = 1;
        if (partials_out) memset(partials_out, 0, g * (size_t)LWKZG_CELL_VERIFY_PARTIAL_BYTES);
        complete_now(res, C_KZG_OK, true);
        return C_KZG_OK;
    }
    const int mode = mode_of(v->s);
    ensure_lagrange(v->ctx, mode);   // (a load unless the mode changed to c-kzg after the verifier was made)
    std::lock_guard<std::mutex> enq(v->enq_mu);
    return async_enqueue(v, res, n, mode, caller, [&](Ctx *c, AsyncJob *j, int *hf) {
        GroupCall &gc = v->gcall[j - v->ring.slots];   // the slot's own: no call in flight reads it
        gc.ok_out = ok_out, gc.rc_out = rc_out, gc.partials_out = partials_out, gc.g = g;
        for (size_t k = 0; k <= g; k++) gc.h_off[k] = (uint32_t)offsets[k];
        return enqueue_groups_on(v, c, j, CallItems{comms, cells, proofs, idx}, caller, hf);
    });
}

// ---- blob calls: the checks of the item calls with blobs for items, then the same two enqueue functions ----
// what both blob calls decide first: async_enqueue_checks, then that the verifier takes blobs, and nb of them
C_KZG_RET blob_enqueue_checks(CellVerifier **out, const LwkzgCellVerifier *handle, LwkzgCellVerifyResult *res, size_t nb, const char *fn) {
    AsyncVerifier *base;
    const C_KZG_RET refused = async_enqueue_checks(&base, handle, kCellVerifierMagic, res, 0, fn, "blobs");
    if (refused != C_KZG_OK) return refused;
    CellVerifier *v = *out = static_cast<CellVerifier *>(base);
    if (v->bcap == 0 || nb > v->bcap) {
        set_error(v->bcap ? "%s: %zu blobs, the verifier was created for %zu" : "%s: the verifier was not created by lwkzg_cell_verifier_new_blobs and has no scratch for the cells of blobs",
                  fn, nb, v->bcap);
        return async_refuse(res, C_KZG_BADARGS);
    }
    return C_KZG_OK;
}

C_KZG_RET cell_verifier_enqueue_blobs_impl(const LwkzgCellVerifier *handle, LwkzgCellVerifyResult *res, const uint8_t *blobs, const uint8_t *comms,
                                           const uint8_t *proofs, size_t nb, hipStream_t caller) {
    const char *fn = "lwkzg_cell_verifier_enqueue_blobs";
    CellVerifier *v;
    const C_KZG_RET refused = blob_enqueue_checks(&v, handle, res, nb, fn);
    if (refused != C_KZG_OK) return refused;
    if (nb == 0) {   // the batch call's answer to no items
        complete_now(res, C_KZG_OK, true);
        return C_KZG_OK;
    }
    if (!blobs || !comms || !proofs) {
        set_error("%s: NULL argument", fn);
        return async_refuse(res, C_KZG_BADARGS);
    }
    const int mode = mode_of(v->s);
    ensure_lagrange(v->ctx, mode);
    std::lock_guard<std::mutex> enq(v->enq_mu);
    return async_enqueue(v, res, nb * kCellsPerBlob, mode, caller, [&](Ctx *c, AsyncJob *j, int *hf) {
        return enqueue_on(v, c, j, CallItems{comms, nullptr, proofs, nullptr, blobs, nb}, caller, hf);
    });
}

C_KZG_RET cell_verifier_enqueue_blobs_groups_impl(const LwkzgCellVerifier *handle, LwkzgCellVerifyResult *res, uint8_t *ok_out, int32_t *rc_out,
                                                  uint8_t *partials_out, const uint8_t *blobs, const uint8_t *comms, const uint8_t *proofs,
                                                  size_t nb, const uint64_t *offsets, size_t g, hipStream_t caller) {
    const char *fn = "lwkzg_cell_verifier_enqueue_blobs_groups";
    CellVerifier *v;
    const C_KZG_RET refused = blob_enqueue_checks(&v, handle, res, nb, fn);
    if (refused != C_KZG_OK) return refused;
    if (v->gcap == 0 || g > v->gcap) {
        set_error(v->gcap ? "%s: %zu groups, the verifier was created for %zu" : "%s: the verifier was created without groups (max_groups == 0)", fn,
                  g, v->gcap);
        return async_refuse(res, C_KZG_BADARGS);
    }
    if ((g > 0 && (!ok_out || !rc_out || !offsets)) || (nb > 0 && (!blobs || !comms || !proofs))) {
        set_error("%s: NULL argument", fn);
        return async_refuse(res, C_KZG_BADARGS);
    }
    if (!group_offsets_valid(offsets, g, nb)) {
        set_error("%s: group_offsets must be %zu ascending values from 0 to %zu (blobs)", fn, g + 1, nb);
        return async_refuse(res, C_KZG_BADARGS);
    }
    if (nb == 0) {   // no group, or empty groups alone: the batch call's answer to n == 0 for each
        for (size_t j = 0; j < g; j++) rc_out[j] = (int32_t)C_KZG_OK, ok_out[j] = 1;
        if (partials_out) memset(partials_out, 0, g * (size_t)LWKZG_CELL_VERIFY_PARTIAL_BYTES);
        complete_now(res, C_KZG_OK, true);
        return C_KZG_OK;
    }
    const int mode = mode_of(v->s);
    ensure_lagrange(v->ctx, mode);
    std::lock_guard<std::mutex> enq(v->enq_mu);
    return async_enqueue(v, res, nb * kCellsPerBlob, mode, caller, [&](Ctx *c, AsyncJob *j, int *hf) {
        GroupCall &gc = v->gcall[j - v->ring.slots];   // the slot's own: no call in flight reads it
        gc.ok_out = ok_out, gc.rc_out = rc_out, gc.partials_out = partials_out, gc.g = g;
        for (size_t k = 0; k <= g; k++) gc.h_off[k] = (uint32_t)(offsets[k] * kCellsPerBlob);   // in ITEMS, as every reader takes them
        return enqueue_groups_on(v, c, j, CallItems{comms, nullptr, proofs, nullptr, blobs, nb}, caller, hf);
    });
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_cell_verifier_new(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_cells) {
    return guarded("lwkzg_cell_verifier_new", [&] { return cell_verifier_new_impl(out, s, max_cells, 0); });
}

C_KZG_RET lwkzg_cell_verifier_new_groups(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_cells, size_t max_groups) {
    return guarded("lwkzg_cell_verifier_new_groups", [&] {
        if (max_groups == 0) {
            if (out) *out = nullptr;
            return C_KZG_BADARGS;
        }
        return cell_verifier_new_impl(out, s, max_cells, max_groups);
    });
}

C_KZG_RET lwkzg_cell_verifier_enqueue_groups(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, uint8_t *ok_out, int32_t *rc_out,
                                             uint8_t *partials_out, const void *commitments48_dev, const void *cell_indices_dev,
                                             const void *cells_dev, const void *proofs48_dev, size_t n, const uint64_t *group_offsets, size_t g,
                                             void *stream) {
    return guarded("lwkzg_cell_verifier_enqueue_groups", [&] {
        return cell_verifier_enqueue_groups_impl(v, result, ok_out, rc_out, partials_out, (const uint8_t *)commitments48_dev,
                                                 (const uint64_t *)cell_indices_dev, (const uint8_t *)cells_dev, (const uint8_t *)proofs48_dev, n,
                                                 group_offsets, g, (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_cell_verifier_enqueue(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, const void *commitments48_dev,
                                      const void *cell_indices_dev, const void *cells_dev, const void *proofs48_dev, size_t n, void *stream) {
    return guarded("lwkzg_cell_verifier_enqueue", [&] {
        return cell_verifier_enqueue_impl(v, result, (const uint8_t *)commitments48_dev, (const uint64_t *)cell_indices_dev,
                                          (const uint8_t *)cells_dev, (const uint8_t *)proofs48_dev, n, (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_cell_verifier_new_blobs(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_blobs, size_t max_groups) {
    return guarded("lwkzg_cell_verifier_new_blobs", [&] {
        if (max_blobs == 0 || max_blobs > kBlobGroupCap) {   // one extension chunk, one workgroup's grouping
            if (out) *out = nullptr;
            if (out && s) set_error("lwkzg_cell_verifier_new_blobs: max_blobs must be 1 .. %u", kBlobGroupCap);
            return C_KZG_BADARGS;
        }
        return cell_verifier_new_impl(out, s, max_blobs * kCellsPerBlob, max_groups, max_blobs);
    });
}

C_KZG_RET lwkzg_cell_verifier_enqueue_blobs(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, const void *blobs_dev, const void *commitments48_dev,
                                            const void *cell_proofs48_dev, size_t n, void *stream) {
    return guarded("lwkzg_cell_verifier_enqueue_blobs", [&] {
        return cell_verifier_enqueue_blobs_impl(v, result, (const uint8_t *)blobs_dev, (const uint8_t *)commitments48_dev,
                                                (const uint8_t *)cell_proofs48_dev, n, (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_cell_verifier_enqueue_blobs_groups(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, uint8_t *ok_out, int32_t *rc_out,
                                                   uint8_t *partials_out, const void *blobs_dev, const void *commitments48_dev,
                                                   const void *cell_proofs48_dev, size_t n, const uint64_t *group_offsets, size_t g,
                                                   void *stream) {
    return guarded("lwkzg_cell_verifier_enqueue_blobs_groups", [&] {
        return cell_verifier_enqueue_blobs_groups_impl(v, result, ok_out, rc_out, partials_out, (const uint8_t *)blobs_dev,
                                                       (const uint8_t *)commitments48_dev, (const uint8_t *)cell_proofs48_dev, n, group_offsets,
                                                       g, (hipStream_t)stream);
    });
}

int lwkzg_cell_verifier_pending(const LwkzgCellVerifier *v) { return async_verifier_pending(v, kCellVerifierMagic); }
C_KZG_RET lwkzg_cell_verifier_wait(LwkzgCellVerifier *v) { return async_verifier_wait(v, kCellVerifierMagic); }
void lwkzg_cell_verifier_free(LwkzgCellVerifier *v) { async_verifier_free<CellVerifier>(v, kCellVerifierMagic); }

C_KZG_RET lwkzg_cell_verifier_host_steps(LwkzgCellVerifyResult *out, const uint8_t *distinct48, size_t m, const uint8_t *digests32, size_t n,
                                         uint32_t bad_index, const int32_t *status, const uint32_t *first_item, const uint8_t *sums3x97,
                                         const uint8_t *rli48, const KZGSettings *s, int mode) {
    if (!out) return C_KZG_BADARGS;
    memset(out, 0, sizeof *out);
    out->first_bad = kNoneBad;
    out->m = (uint32_t)m;
    auto refuse = [&] { return async_refuse(out, C_KZG_BADARGS); };
    if (!mode_known(mode)) return refuse();
    if (n == 0 || m == 0 || m > n) return refuse();
    // what each outcome reads: a bad index nothing; a fault word the words and first_item; an honest batch everything
    if (bad_index == kNoneBad && (!status || !first_item)) return refuse();
    const bool rejected = bad_index != kNoneBad || first_fault(status, status + n, first_item, n, m) != kNoneBad;
    if (!rejected && (!distinct48 || !digests32 || !sums3x97 || !rli48 || !s || !s->g2_values)) return refuse();
    C_KZG_RET rc = C_KZG_ERROR;
    bool ok = false;
    try {
        uint32_t r_raw[8];
        int32_t code = 0;
        if (!decide_or_challenge(r_raw, &out->first_bad, &code, distinct48, m, digests32, n, bad_index, status, status ? status + n : nullptr,
                                 first_item, mode)) {
            complete_now(out, (C_KZG_RET)code, false);   // a rejected batch: the code, and nothing behind r is read
            return C_KZG_OK;
        }
        Fr pw[33];
        cell_batch_powers(pw, r_raw);   // (step 1's other product; the device takes it)
        cell_r_bytes(out->partials, r_raw, mode);
        uint8_t sums[3][96];
        int infs[3];
        rc = sums_from_97(sums, infs, sums3x97) ? cell_batch_finish(&ok, out->partials + 32, sums, infs, rli48, s) : C_KZG_BADARGS;
    } catch (...) {
        rc = C_KZG_ERROR;
    }
    if (rc != C_KZG_OK) memset(out->partials, 0, sizeof out->partials);
    complete_now(out, rc, ok && rc == C_KZG_OK);
    return C_KZG_OK;
}

C_KZG_RET lwkzg_cell_verifier_groups_host_steps(LwkzgCellVerifyResult *out, uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out,
                                                const uint64_t *group_offsets, size_t g, size_t n, const uint32_t *row_base,
                                                const uint32_t *bad_words, const int32_t *status, const uint32_t *first_item,
                                                const uint8_t *digests32, const uint8_t *distinct48, const uint8_t *sums3x97,
                                                const uint8_t *rli48, const KZGSettings *s, int mode) {
    if (!out) return C_KZG_BADARGS;
    memset(out, 0, sizeof *out);
    out->first_bad = kNoneBad;
    auto refuse = [&] { return async_refuse(out, C_KZG_BADARGS); };
    if (!mode_known(mode) || g == 0 || n == 0 || n > 0x7fffffffu || g > 0x40000000u) return refuse();
    if (!ok_out || !rc_out || !row_base || !bad_words || !group_offsets_valid(group_offsets, g, n)) return refuse();
    return guarded("lwkzg_cell_verifier_groups_host_steps", [&] {
        std::vector<uint32_t> off(g + 1), r_raw(8 * g), flags(g);
        std::vector<int32_t> rc(g);
        std::vector<Fr> pw(kPwWords * g);
        for (size_t j = 0; j <= g; j++) off[j] = (uint32_t)group_offsets[j];
        // what each outcome reads: a bad word nothing; a fault word the words and first_item; an honest group everything
        bool honest = false;
        for (size_t j = 0; j < g; j++) {
            if (off[j] == off[j + 1] || bad_words[j]) continue;
            if (!status || !first_item) return refuse();
            const uint32_t rb = row_base[j], m = row_base[j + 1] - rb;
            if (row_base[j + 1] < rb || row_base[j + 1] > n || m > off[j + 1] - off[j]) return refuse();
            honest = honest || first_fault(status + off[j], status + n + rb, first_item + rb, off[j + 1] - off[j], m) == kNoneBad;
        }
        if (honest && (!digests32 || !distinct48 || !sums3x97 || !rli48 || !s || !s->g2_values)) return refuse();
        groups_decide(rc.data(), r_raw.data(), pw.data(), flags.data(), off.data(), g, n, row_base, bad_words, status, first_item, digests32,
                      distinct48, mode);
        groups_finish(out, ok_out, rc_out, partials_out, rc.data(), r_raw.data(), flags.data(), off.data(), g, row_base[g], s, mode, false,
                      [&](size_t j, uint8_t sums[3][96], int infs[3], uint8_t rli[48]) {
                          memcpy(rli, rli48 + 48 * j, 48);
                          return sums_from_97(sums, infs, sums3x97 + 3 * 97 * j);
                      });
        return C_KZG_OK;
    });
}

}  // extern "C"
