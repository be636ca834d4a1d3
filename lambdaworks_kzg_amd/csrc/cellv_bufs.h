// cellv_bufs.h -- the device side of a cell proof batch, carved out of one allocation: shared by the synchronous calls
// (cells_verify_api.hip and cells_verify_groups.hip, a grow-only block each with the context) and the asynchronous verifier
// (cells_verify_async.hip, a block of its own). What a grouped call keeps beside it is CellgBufs (cells_verify_groups.h).
#pragma once
#include "carve.h"
#include "cells_common.h"
#include "knobs.h"

#include <chrono>

namespace lwk {

struct CellvBufs {
    uint8_t *cells, *proofs, *comm_in, *canon_p, *canon_c, *digests, *out96, *rli48;
    uint64_t *idx;
    uint32_t *rows, *perm_row, *row_off, *perm_col, *col_off, *verdict_p, *verdict_c, *sc_a, *sc_b, *sc_c;
    int32_t *kind_p, *kind_c, *status, *inf;
    G1Affine29 *pts_p, *pts_c, *tab_p, *tab_c;
    G1Xyzz29 *vm_tmp, *partial, *bsum;
    F29<2> *vm_pre;
    Fr *a_mont, *pw, *colcoef;
};

constexpr size_t kCellvPwSlots = 34;   // Fr-sized slots of pw: the 33 powers, then a slot for the asynchronous verifier's skip word

// staging: room for the cells, proofs and indices of a host-pointer call (a verifier reads its inputs where they are). batch: what the
// batch call alone runs behind r -- its one set of sums, the byte-spaced tables of vmsm.hip, one power table, one interpolant's scratch
// (a grouped call has CellgBufs for that). groups: the column lists, 128 each (a grouped call has one per group)
inline void cellv_carve(CellvBufs &b, Carver &cv, size_t cap, bool staging = true, bool batch = true, size_t groups = 1) {
    cv.take(b.cells, staging ? cap * kCellBytes : 0);
    cv.take(b.proofs, staging ? cap * 48 : 0);
    cv.take(b.comm_in, cap * 48);
    cv.take(b.canon_p, cap * 48);
    cv.take(b.canon_c, cap * 48);
    cv.take(b.digests, cap * 32);
    cv.take(b.out96, batch ? 3 * 96 : 0);
    cv.take(b.rli48, batch ? 48 : 0);
    cv.take(b.idx, staging ? cap * 8 : 0);
    cv.take(b.rows, cap * 4);
    cv.take(b.perm_row, cap * 4);
    cv.take(b.row_off, (cap + 1) * 4);
    cv.take(b.perm_col, cap * 4);
    cv.take(b.col_off, (groups * kCellsPerBlob + 1) * 4);
    cv.take(b.verdict_p, cap * 4);
    cv.take(b.verdict_c, cap * 4);
    cv.take(b.sc_a, cap * 32);
    cv.take(b.sc_b, cap * 32);
    cv.take(b.sc_c, cap * 32);
    cv.take(b.kind_p, cap * 4);
    cv.take(b.kind_c, cap * 4);
    cv.take(b.status, cap * 4);
    cv.take(b.inf, batch ? 3 * 4 : 0);
    cv.take(b.pts_p, cap * sizeof(G1Affine29));
    cv.take(b.pts_c, cap * sizeof(G1Affine29));
    cv.take(b.tab_p, batch ? cap * kVmsmRows * sizeof(G1Affine29) : 0);
    cv.take(b.tab_c, batch ? cap * kVmsmRows * sizeof(G1Affine29) : 0);
    cv.take(b.vm_tmp, batch ? cap * 2 * kVmsmSteps * sizeof(G1Xyzz29) : 0);
    cv.take(b.partial, batch ? 3 * vmsm_max_slices(cap) * 256 * sizeof(G1Xyzz29) : 0);
    cv.take(b.bsum, batch ? 3 * 256 * sizeof(G1Xyzz29) : 0);
    cv.take(b.vm_pre, batch ? cap * 2 * kVmsmSteps * sizeof(F29<2>) : 0);
    cv.take(b.a_mont, cap * sizeof(Fr));
    cv.take(b.pw, batch ? kCellvPwSlots * sizeof(Fr) : 0);
    cv.take(b.colcoef, batch ? (size_t)kCellsPerBlob * kCellElems * sizeof(Fr) : 0);
}
inline size_t cellv_carve(CellvBufs &b, uint8_t *base, size_t cap) {   // the batch call's whole block
    Carver cv(base);
    cellv_carve(b, cv, cap);
    return cv.bytes();
}

// ---- what the synchronous calls over these buffers share (cells_verify_api.hip, cells_verify_groups.hip) --------------------------------
struct PhaseClock {   // LWKZG_TIMING=1: device time between the phases' boundaries on the call's stream, host time beside it
    static constexpr int kMarks = 8;
    hipEvent_t ev[kMarks] = {};
    bool on = false;
    hipStream_t st = nullptr;
    void begin(hipStream_t s) {
        on = knobs().timing;
        st = s;
        if (!on) return;
        for (auto &e : ev)
            if (hipEventCreate(&e) != hipSuccess) on = false;
    }
    void mark(int k) {
        if (on) hipEventRecord(ev[k], st);
    }
    float ms(int a, int b) {
        float t = 0;
        return on && hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? t : -1.f;
    }
    ~PhaseClock() {
        for (auto &e : ev)
            if (e) hipEventDestroy(e);
    }
};

inline double wall_ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

}  // namespace lwk
