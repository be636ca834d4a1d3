// cells_verify_api.hip -- EIP-7594 verify_cell_kzg_proof_batch: lwkzg_verify_cell_kzg_proof_batch (+ _device), lwkzg_cell_verify_partials,
// lwkzg_cell_batch_challenge_host. DESIGN.md section 4i.
//
// One call, one stream, two host visits:
//   host     indices checked (< 128), commitments de-duplicated by byte equality in order of first occurrence (m rows), the items
//            counting-sorted by row and by column (the host holds the 48 n + 8 n bytes anyway: the device form copies them down)
//   device   both point sets validated (the m distinct commitments padded with infinity encodings to the proofs' n, so that the
//            two-set launches of the blob batch serve), the per-cell digests and the element range check; digests and status come down
//   device   beside the host's hash: the byte-spaced rows of both point sets (k_vmsm_multiples)
//   host     r from the distinct commitments and the digests; r^(2^k) goes up
//   device   scalars, row weights, column sums + interpolation, the 64-term MSM on the engine's own launch set, the three
//            variable-base sums (vmsm.hip); four points come down
//   host     the pairing check against g2_values[64] (pairing.hip keeps its line table beside the others)
// This call reports no first_bad and keeps its single status word and its own launch sequence; of the host unit that the calls with
// attribution share (cells_verify_host.h) it takes cell_r_bytes, and sums_from_pinned of async_verifier.h.
#include "abi_guard.h"
#include "cell_groups_plan.h"
#include "cells_verify_blobs.h"
#include "cells_verify_host.h"
#include "cellv_bufs.h"
#include "knobs.h"

#include <string.h>

#include <vector>

namespace lwk {

namespace {

constexpr size_t kItemMsg = 16 + kCellBytes + 48;   // le64(row) | le64(k) | cell | proof
constexpr size_t kPinTail = 33 * sizeof(Fr) + 3 * 96 + 3 * 4 + 48 + 12;   // powers up; three sums, their flags and RLI down

static_assert(kPlanCellsPerBlob == (size_t)kCellsPerBlob, "cell_groups_plan.h groups by the cells of a blob");   // Grouping, group_items: there

typedef CellvBufs Bufs;   // the device side of a batch, carved out of one allocation (cellv_bufs.h)

// grow-only, kept with the settings object: no allocation in steady state (caller holds c->mu)
C_KZG_RET reserve(Ctx *c, size_t n, Bufs &b) {
    if (!c->cellv_ev) LWK_HIP(hipEventCreateWithFlags(&c->cellv_ev, hipEventDisableTiming));
    if (c->cellv.cap < n) {
        size_t bytes = 0;
        C_KZG_RET rc = grow_reserve(c->cellv, n, 256, [&](size_t cap) { Bufs probe; return bytes = cellv_carve(probe, nullptr, cap); }, nullptr);
        if (rc == C_KZG_ERROR) return rc;   // the wait failed: both buffers are as they were
        if (c->cellv_pin) hipHostFree(c->cellv_pin);
        c->cellv_pin = nullptr;
        if (rc == C_KZG_OK && hipHostMalloc((void **)&c->cellv_pin, c->cellv.cap * 36 + kPinTail) != hipSuccess) {
            (void)hipGetLastError();
            grow_free(c->cellv);
            rc = C_KZG_MALLOC;
        }
        if (rc != C_KZG_OK) {
            set_error("verify_cell_kzg_proof_batch: no memory for a batch of %zu cells (%zu bytes on the device)", n, bytes);
            return rc;
        }
    }
    cellv_carve(b, c->cellv.dev, c->cellv.cap);
    return C_KZG_OK;
}

// r (canonical limbs), the three sums of vmsm.hip and the compressed RLI of a batch. Host pointers are uploaded into the context's
// buffer; device pointers (device_inputs) are read where they are, except the commitments and the indices, which come down first.
// front (cells_verify_blobs.h): the caller makes the items, the lists and the grouping itself; the four item arrays are not read.
C_KZG_RET cell_batch_sums(uint32_t r_raw[8], uint8_t sums[3][96], int infs[3], uint8_t rli48[48], const uint8_t *comms, const uint64_t *idx,
                          const uint8_t *cells, const uint8_t *proofs, size_t n, const KZGSettings *s, int mode, bool device_inputs,
                          hipStream_t caller, const CellFront *front = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    const int le = mode_rules(mode).le();
    Grouping own;
    const Grouping &g = front ? front->g : own;
    if (!front && !device_inputs && !group_items(own, comms, idx, n)) {   // before any device work: decidable without a GPU
        set_error("verify_cell_kzg_proof_batch: a cell index is not below %d", kCellsPerBlob);
        return C_KZG_BADARGS;
    }
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (!s->g2_values) {
        set_error("KZGSettings.g2_values is NULL");
        return C_KZG_ERROR;
    }
    ensure_lagrange(c, mode);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = caller ? caller : c->stream;
    std::vector<uint8_t> h_comms;
    std::vector<uint64_t> h_idx;
    if (device_inputs) {
        h_comms.resize(48 * n);
        h_idx.resize(n);
        LWK_HIP(hipMemcpyAsync(h_comms.data(), comms, 48 * n, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(h_idx.data(), idx, 8 * n, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipStreamSynchronize(st));
        if (!group_items(own, h_comms.data(), h_idx.data(), n)) {
            set_error("verify_cell_kzg_proof_batch: a cell index is not below %d", kCellsPerBlob);
            return C_KZG_BADARGS;
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    Bufs b;
    C_KZG_RET rc = reserve(c, n, b);
    if (rc != C_KZG_OK) return rc;
    if ((rc = ctx_reserve(c, 1)) != C_KZG_OK) return rc;
    WsUse wsu(c, st);
    StreamDrain drain{st};   // nothing of this call is in flight when it returns, whatever the exit
    PhaseClock clk;
    clk.begin(st);
    uint8_t *pin = c->cellv_pin;
    uint8_t *pin_dig = pin, *pin_tail = pin + 36 * c->cellv.cap;
    int32_t *pin_status = (int32_t *)(pin + 32 * c->cellv.cap);

    // the distinct commitments, padded with infinity encodings to the proofs' count: both point sets go through the two-set launches
    std::vector<uint8_t> padded(front ? 0 : 48 * n, 0);
    if (!front) {
        memcpy(padded.data(), g.distinct.data(), 48 * g.m);
        for (size_t j = g.m; j < n; j++) padded[48 * j] = 0xc0;
        LWK_HIP(hipMemcpyAsync(b.comm_in, padded.data(), 48 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.rows, g.rows.data(), 4 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.perm_row, g.perm_row.data(), 4 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.row_off, g.row_off.data(), 4 * (g.m + 1), hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.perm_col, g.perm_col.data(), 4 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.col_off, g.col_off.data(), 4 * (kCellsPerBlob + 1), hipMemcpyHostToDevice, st));
    }
    const uint8_t *d_cells = cells, *d_proofs = proofs;
    const uint64_t *d_idx = idx;
    if (front) {
        if ((rc = front->items(c, st, b, nullptr, d_cells, d_proofs)) != C_KZG_OK) return rc;
        d_idx = b.idx;
    } else if (!device_inputs) {
        LWK_HIP(hipMemcpyAsync(b.cells, cells, n * kCellBytes, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.proofs, proofs, 48 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.idx, idx, 8 * n, hipMemcpyHostToDevice, st));
        d_cells = b.cells, d_proofs = b.proofs, d_idx = b.idx;
    }
    LWK_HIP(hipMemsetAsync(b.status, 0, 4 * n, st));
    LWK_HIP(hipMemsetAsync(b.sc_c, 0, 32 * n, st));
    clk.mark(0);
    const int bad = (int)bad_input(mode);
    launch_cellv_digests(d_cells, d_proofs, b.rows, d_idx, b.digests, b.status, bad, le, n, st);
    clk.mark(1);
    const PointSet set_p{d_proofs, b.pts_p, b.kind_p, b.canon_p, b.verdict_p}, set_c{b.comm_in, b.pts_c, b.kind_c, b.canon_c, b.verdict_c};
    launch_decompress_points(set_p, &set_c, n, st);
    launch_subgroup_canon(set_p, &set_c, b.status, bad, n, st, false, true);
    if (front) front->fold_status(b.status, bad, st);
    clk.mark(2);
    LWK_HIP(hipMemcpyAsync(pin_dig, b.digests, 32 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(pin_status, b.status, 4 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipEventRecord(c->cellv_ev, st));
    launch_vmsm_multiples2(b.pts_p, b.kind_p, b.tab_p, b.pts_c, b.kind_c, b.tab_c, b.vm_tmp, b.vm_pre, n, st);   // beside the host's hash
    LWK_HIP(hipEventSynchronize(c->cellv_ev));
    const auto t2 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < n; i++)
        if (pin_status[i] != 0) {
            set_error("verify_cell_kzg_proof_batch: a commitment or a proof is not a point of G1, or a cell element is not below r (first at %zu)%s", i,
                      front ? ", or the front rejected the item's blob" : "");
            return bad_input(mode);
        }
    cell_batch_challenge(r_raw, g.distinct.data(), g.m, pin_dig, n, le);
    cell_batch_powers((Fr *)pin_tail, r_raw);
    const auto t3 = std::chrono::steady_clock::now();
    LWK_HIP(hipMemcpyAsync(b.pw, pin_tail, 33 * sizeof(Fr), hipMemcpyHostToDevice, st));
    clk.mark(3);
    launch_cellv_scalars(b.pw, d_idx, c->tw_fwd, b.a_mont, b.sc_a, b.sc_b, b.perm_row, b.row_off, b.sc_c, n, g.m, st);
    launch_cellv_interpolant(d_cells, b.a_mont, b.perm_col, b.col_off, c->tw_inv, b.colcoef, c->ws.scalars2, le, st);
    clk.mark(4);
    const bool lg = coefficients_to_msm_form(c, mode, 1, st);
    msm_stages(c, c->ws.scalars2, b.rli48, 1, st, 0, false, lg);
    clk.mark(5);
    launch_vmsm_accumulate(b.sc_a, b.sc_b, b.tab_p, b.kind_p, b.tab_c, b.kind_c, b.partial, n, st, b.sc_c);
    launch_vmsm_reduce(b.partial, b.bsum, b.out96, b.inf, n, st);
    clk.mark(6);
    uint8_t *res = pin_tail + 33 * sizeof(Fr);
    LWK_HIP(hipMemcpyAsync(res, b.out96, 3 * 96, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(res + 3 * 96, b.inf, 3 * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(res + 3 * 96 + 12, b.rli48, 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipGetLastError());
    LWK_HIP(hipStreamSynchronize(st));
    sums_from_pinned(sums, infs, res, res + 3 * 96);
    memcpy(rli48, res + 3 * 96 + 12, 48);
    if (clk.on)
        fprintf(stderr, "[lambdaworks_kzg_amd] verify cells n=%zu m=%zu: host grouping %.3f ms | device: digests %.3f, validation %.3f, "
                        "rows beside the hash + wait %.3f, scalars + column sums %.3f, 64-term MSM %.3f, linear combinations %.3f ms | "
                        "host: until digests landed %.3f, final hash + powers %.3f, total before the pairing %.3f ms\n",
                n, g.m, wall_ms(t0, t1), clk.ms(0, 1), clk.ms(1, 2), clk.ms(2, 3), clk.ms(3, 4), clk.ms(4, 5), clk.ms(5, 6), wall_ms(t1, t2),
                wall_ms(t2, t3), wall_ms(t0, std::chrono::steady_clock::now()));
    return C_KZG_OK;
}

// the verdict (ok) and / or r and the four sums (partials): one code path up to the pairing
C_KZG_RET cell_batch_impl(bool *ok, uint8_t *partials, const void *comms, const void *idx, const void *cells, const void *proofs, size_t n,
                          const KZGSettings *s, bool device_inputs, hipStream_t caller, const CellFront *front = nullptr) {
    if (!s) return C_KZG_BADARGS;
    const int mode = mode_of(s);
    if (n == 0) {
        if (ok) *ok = true;   // the consensus specs' and c-kzg-4844 2.x's rule for cells, in both modes
        return C_KZG_OK;
    }
    if (!front && (!comms || !idx || !cells || !proofs)) {
        set_error("verify_cell_kzg_proof_batch: NULL argument");
        return C_KZG_BADARGS;
    }
    uint32_t r_raw[8];
    uint8_t sums[3][96], rli48[48];
    int infs[3];
    C_KZG_RET rc = cell_batch_sums(r_raw, sums, infs, rli48, (const uint8_t *)comms, (const uint64_t *)idx, (const uint8_t *)cells,
                                   (const uint8_t *)proofs, n, s, mode, device_inputs, caller, front);
    if (rc != C_KZG_OK) return rc;
    if (partials) cell_r_bytes(partials, r_raw, mode);
    const auto t0 = std::chrono::steady_clock::now();
    rc = cell_batch_finish(ok, partials ? partials + 32 : nullptr, sums, infs, rli48, s);
    if (knobs().timing && ok)
        fprintf(stderr, "[lambdaworks_kzg_amd] verify cells n=%zu: pairing side %.3f ms\n", n, wall_ms(t0, std::chrono::steady_clock::now()));
    return rc;
}

}  // namespace

// cells_verify_blobs.h
C_KZG_RET cell_batch_front(bool *ok, uint8_t *partials, size_t n, const KZGSettings *s, hipStream_t caller, const CellFront &front) {
    return cell_batch_impl(ok, partials, nullptr, nullptr, nullptr, nullptr, n, s, false, caller, &front);
}

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_verify_cell_kzg_proof_batch(bool *ok, const Bytes48 *commitments, const uint64_t *cell_indices, const Cell *cells,
                                            const Bytes48 *proofs, size_t n, const KZGSettings *s) {
    if (!ok) return C_KZG_BADARGS;
    *ok = false;
    return guarded("lwkzg_verify_cell_kzg_proof_batch",
                   [&] { return cell_batch_impl(ok, nullptr, commitments, cell_indices, cells, proofs, n, s, false, nullptr); });
}

C_KZG_RET lwkzg_verify_cell_kzg_proof_batch_device(bool *ok, const void *commitments48_dev, const void *cell_indices_dev, const void *cells_dev,
                                                   const void *proofs48_dev, size_t n, const KZGSettings *s, void *stream) {
    if (!ok) return C_KZG_BADARGS;
    *ok = false;
    return guarded("lwkzg_verify_cell_kzg_proof_batch_device", [&] {
        return cell_batch_impl(ok, nullptr, commitments48_dev, cell_indices_dev, cells_dev, proofs48_dev, n, s, true, (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_cell_verify_partials(uint8_t *out, const Bytes48 *commitments, const uint64_t *cell_indices, const Cell *cells,
                                     const Bytes48 *proofs, size_t n, const KZGSettings *s) {
    if (!out && n) return C_KZG_BADARGS;
    return guarded("lwkzg_cell_verify_partials",
                   [&] { return cell_batch_impl(nullptr, out, commitments, cell_indices, cells, proofs, n, s, false, nullptr); });
}

C_KZG_RET lwkzg_cell_batch_challenge_host(uint8_t r_out[32], const Bytes48 *commitments, const uint64_t *cell_indices, const Cell *cells,
                                          const Bytes48 *proofs, size_t n, int mode) {
    if (!r_out || !mode_known(mode)) return C_KZG_BADARGS;
    if (n && (!commitments || !cell_indices || !cells || !proofs)) return C_KZG_BADARGS;
    return guarded("lwkzg_cell_batch_challenge_host", [&]() -> C_KZG_RET {
        Grouping g;
        if (!group_items(g, (const uint8_t *)commitments, cell_indices, n)) return C_KZG_BADARGS;
        std::vector<uint8_t> digests(32 * n), msg(kItemMsg);
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 8; k++) {
                msg[k] = (uint8_t)((uint64_t)g.rows[i] >> (8 * k));
                msg[8 + k] = (uint8_t)(cell_indices[i] >> (8 * k));
            }
            memcpy(&msg[16], cells[i].bytes, kCellBytes);
            memcpy(&msg[16 + kCellBytes], proofs[i].bytes, 48);
            sha256_fast(&digests[32 * i], msg.data(), msg.size());
        }
        uint32_t r_raw[8];
        cell_batch_challenge(r_raw, g.distinct.data(), g.m, digests.data(), n, mode_rules(mode).little_endian);
        cell_r_bytes(r_out, r_raw, mode);
        return C_KZG_OK;
    });
}

}  // extern "C"
