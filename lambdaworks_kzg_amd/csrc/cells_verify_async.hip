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
// async_verifier.h, shared with verify_async.hip.
#include "abi_guard.h"
#include "async_verifier.h"
#include "cell_group.cuh"
#include "cellv_bufs.h"

#include <chrono>
#include <new>
#include <random>

namespace lwk {

namespace {

constexpr uint64_t kCellVerifierMagic = 0x4c574b5a43564659ull;  // "LWKZCVFY"
constexpr size_t kPinPowers = 33 * sizeof(Fr) + 4;   // the powers and, behind them, the skip word: one copy up
constexpr size_t kPinSums = 3 * 96 + 3 * 4 + 48;     // the three sums, their flags, RLI: 348 bytes down

struct CellVerifier : AsyncVerifier {
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
    const size_t used = cellv_carve(v->b, base, v->cap, false);
    Carver cv(base ? base + used : nullptr);
    cell_group_carve(v->g, cv, v->cap, v->slots);
    cv.take(v->fault, 2 * v->cap * 4);
    v->g.rows = v->b.rows;
    v->g.perm_row = v->b.perm_row;
    v->g.row_off = v->b.row_off;
    v->g.perm_col = v->b.perm_col;
    v->g.col_off = v->b.col_off;
    v->g.distinct = v->b.comm_in;
    return used + cv.bytes();
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
    return cv.bytes();
}

// the lowest item at fault: an item's own word (a cell element, its proof), or a distinct commitment's at the item it was first seen at
uint32_t first_fault(const int32_t *fault, const uint32_t *first_item, size_t n, size_t m) {
    uint32_t bad = kNoneBad;
    for (size_t i = 0; i < n; i++)
        if (fault[i] != 0) {
            bad = (uint32_t)i;
            break;
        }
    for (size_t j = 0; j < m; j++)
        if (fault[n + j] != 0 && first_item[j] < bad) bad = first_item[j];
    return bad;
}

// Host function 1's work on plain blocks (also lwkzg_cell_verifier_host_steps'): the code and first_bad of a rejected batch, or r into
// r_raw and true. bad_index: the lowest i with an index >= 128 (kNoneBad: none), decided first, whatever else is wrong
bool decide_or_challenge(uint32_t r_raw[8], uint32_t *first_bad, int32_t *rc, const uint8_t *distinct48, size_t m, const uint8_t *digests32,
                         size_t n, uint32_t bad_index, const int32_t *fault, const uint32_t *first_item, int mode) {
    if (bad_index != kNoneBad) {
        *first_bad = bad_index;
        *rc = C_KZG_BADARGS;
        return false;
    }
    *first_bad = first_fault(fault, first_item, n, m);
    if (*first_bad != kNoneBad) {
        *rc = bad_input(mode);
        return false;
    }
    cell_batch_challenge(r_raw, distinct48, m, digests32, n, mode_rules(mode).little_endian);
    return true;
}

void r_bytes(uint8_t out32[32], const uint32_t r_raw[8], int mode) {
    if (mode_rules(mode).little_endian) raw_to_le<8>(out32, r_raw);
    else raw_to_be<8>(out32, r_raw);
}

// ---- the two host functions ------------------------------------------------------------------------------------------------------
// Their rules are async_verifier.h's. What they call keeps to them: cell_batch_challenge and cell_batch_powers hash and multiply;
// cell_batch_finish's pairing takes fixed_q_lines' cache mutex (pairing.hip), which guards a search and a push_back and is never held
// across a wait for the GPU or across the lines' computation; its two set_error calls (a NULL g2_values, an interpolant's commitment
// that is no point) cannot happen with a verifier's own copy of the G2 points and the engine's own compressed output, and would only
// write the runtime thread's own error text.

// behind the copies of the head, the fault words, the digests and the padded commitments
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
            if (decide_or_challenge(r_raw, &j->first_bad, &j->code, v->h_comm, m, v->h_dig, j->n, bad_index, v->h_fault, v->h_first, j->mode)) {
                cell_batch_powers((Fr *)v->h_up, r_raw);
                r_bytes(((LwkzgCellVerifyResult *)j->res)->partials, r_raw, j->mode);
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

// the workspace a call on context c takes: one MSM slot
C_KZG_RET reserve_for(Ctx *c) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    C_KZG_RET rc = ctx_reserve(c, 1);
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

C_KZG_RET cell_verifier_new_impl(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_cells) {
    if (!out) return C_KZG_BADARGS;
    *out = nullptr;
    if (!s || max_cells == 0 || max_cells >= 0x40000000u) return C_KZG_BADARGS;
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
    v->seed = draw_seed(v);
    memset(v->g2, 0, sizeof v->g2);
    v->g2[0] = s->g2_values[0];
    v->g2[64] = s->g2_values[64];
    v->own.fs = nullptr;
    v->own.g1_values = nullptr;
    v->own.g2_values = v->g2;
    C_KZG_RET rc = reserve_for(c);
    if (rc == C_KZG_OK)
        if (Ctx *t = c->twin.load(std::memory_order_acquire)) rc = reserve_for(t);
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

// everything of one call on context c, enqueued; caller holds c->mu. *hf: host functions handed to the runtime so far
C_KZG_RET enqueue_on(CellVerifier *v, Ctx *c, AsyncJob *j, const uint8_t *comms, const uint64_t *idx, const uint8_t *cells, const uint8_t *proofs,
                     hipStream_t caller, int *hf) {
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
    LWK_HIP(hipMemsetAsync(v->fault, 0, 4 * n, st));
    LWK_HIP(hipMemsetAsync(b.status, 0, 4 * n, st));
    LWK_HIP(hipMemsetAsync(b.sc_c, 0, 32 * n, st));
    launch_cell_group(comms, idx, n, v->slots, v->seed, 0xffffffffu, v->g, st);
    launch_cellv_digests(cells, proofs, b.rows, idx, b.digests, v->fault, bad, le, n, st);
    const PointSet set_p{proofs, b.pts_p, b.kind_p, b.canon_p, b.verdict_p}, set_c{b.comm_in, b.pts_c, b.kind_c, b.canon_c, b.verdict_c};
    launch_decompress_points(set_p, &set_c, n, st);
    launch_subgroup_canon(set_p, &set_c, b.status, bad, n, st);
    launch_cellv_fault_words(v->fault, b.kind_p, b.kind_c, bad, n, st);
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
                         [&](Ctx *c, AsyncJob *j, int *hf) { return enqueue_on(v, c, j, comms, idx, cells, proofs, caller, hf); });
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_cell_verifier_new(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_cells) {
    return guarded("lwkzg_cell_verifier_new", [&] { return cell_verifier_new_impl(out, s, max_cells); });
}

C_KZG_RET lwkzg_cell_verifier_enqueue(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, const void *commitments48_dev,
                                      const void *cell_indices_dev, const void *cells_dev, const void *proofs48_dev, size_t n, void *stream) {
    return guarded("lwkzg_cell_verifier_enqueue", [&] {
        return cell_verifier_enqueue_impl(v, result, (const uint8_t *)commitments48_dev, (const uint64_t *)cell_indices_dev,
                                          (const uint8_t *)cells_dev, (const uint8_t *)proofs48_dev, n, (hipStream_t)stream);
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
    const bool rejected = bad_index != kNoneBad || first_fault(status, first_item, n, m) != kNoneBad;
    if (!rejected && (!distinct48 || !digests32 || !sums3x97 || !rli48 || !s || !s->g2_values)) return refuse();
    C_KZG_RET rc = C_KZG_ERROR;
    bool ok = false;
    try {
        uint32_t r_raw[8];
        int32_t code = 0;
        if (!decide_or_challenge(r_raw, &out->first_bad, &code, distinct48, m, digests32, n, bad_index, status, first_item, mode)) {
            complete_now(out, (C_KZG_RET)code, false);   // a rejected batch: the code, and nothing behind r is read
            return C_KZG_OK;
        }
        Fr pw[33];
        cell_batch_powers(pw, r_raw);   // (step 1's other product; the device takes it)
        r_bytes(out->partials, r_raw, mode);
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

}  // extern "C"
