// fk20_api.hip -- the FK20 cell proof engine of a settings object (the kernels are fk20.hip): the choice of
// engine (lwkzg_set_cell_proof_engine, lwkzg_cell_proof_engine, lwkzg_fk20_table_bytes, lwkzg_fk20_chunk_blobs), the derivation of the
// 8192 transformed bases and the build of the window table over them, the proof stage that cells_from_coefficients hands a chunk to, and
// the test hook that reads the stage's points (lwkzg_fk20_points).
//
// The bases need no G1 transform: Y^_i[m] = sum_{j <= 62} w^(m j) G[64 (62 - j) + i] is a 4096-term combination of the monomial setup
// with 63 non-zero scalars, so, as the Lagrange form is derived (tables.hip: lagrange_prepare), a kernel writes the scalar rows, the
// settings' own MSM engine commits them 1024 at a time and launch_g1_decompress turns the results back into affine points.
#include "abi_guard.h"
#include "cells_common.h"
#include "fk20.cuh"

#include <string.h>

#include <vector>

namespace lwk {

namespace {

constexpr size_t kHookPoints = kFk20Points + kFk20Terms;   // E and h of one blob
constexpr size_t kHookBytes = kHookPoints * sizeof(G1Xyzz29) + (size_t)kFk20Points * 96 + (size_t)kFk20Points * 4;

void state_free(Fk20State &f) {
    if (f.table) hipFree(f.table);
    if (f.bases) hipFree(f.bases);
    if (f.roots) hipFree(f.roots);
    if (f.pts) hipFree(f.pts);
    if (f.hook_pts) hipFree(f.hook_pts);
    f = Fk20State();
}

// the twin context launches against the same table and scratch: refresh its copies (caller holds both contexts' locks)
void sync_twin(Ctx *c) {
    if (Ctx *t = c->twin.load(std::memory_order_acquire)) t->fk20 = c->fk20;
}

// Everything the engine keeps, into `f`; on failure nothing stays allocated. Caller holds the locks; the device is idle.
C_KZG_RET state_build(Ctx *c, Fk20State &f, int bits) {
    const Fk20Plan plan = fk20_plan(bits);
    C_KZG_RET rc = ctx_reserve(c, kMaxChunk);   // the base derivation's launch sets, and the 2 x 512 slots of a full FK20 chunk
    if (rc != C_KZG_OK) return rc;
    hipStream_t st = c->stream;
    uint8_t *d_comp = nullptr;
    int32_t *d_status = nullptr;
    uint32_t *d_roots_raw = nullptr;
    f.table_bytes = plan.rows * sizeof(G1Affine29);
    bool ok = hipMalloc((void **)&f.table, f.table_bytes) == hipSuccess &&
              hipMalloc((void **)&f.bases, (size_t)kFk20Bases * sizeof(G1Affine)) == hipSuccess &&
              hipMalloc((void **)&f.roots, (size_t)kFk20Roots * kFk20RootDigits) == hipSuccess &&
              hipMalloc((void **)&f.pts, kFk20ChunkBlobs * kFk20Points * sizeof(G1Xyzz29)) == hipSuccess &&
              hipMalloc((void **)&f.hook_pts, kHookBytes) == hipSuccess && hipMalloc((void **)&d_comp, (size_t)kFk20Bases * 48) == hipSuccess &&
              hipMalloc((void **)&d_status, (size_t)kFk20Bases * 4) == hipSuccess &&
              hipMalloc((void **)&d_roots_raw, (size_t)kFk20Points * 32) == hipSuccess;
    std::vector<int32_t> h_status(kFk20Bases, 0);
    bool at_infinity = false;
    if (ok) {
        std::vector<uint32_t> roots_raw((size_t)kFk20Points * 8);
        std::vector<uint8_t> digits((size_t)kFk20Roots * kFk20RootDigits);
        for (int idx = 0; idx < kFk20Roots; idx++) {
            uint32_t raw[8];
            fk20_root_raw(raw, idx);
            if (idx < kFk20Points) memcpy(&roots_raw[(size_t)idx * 8], raw, 32);
            fk20_recode_root(&digits[(size_t)idx * kFk20RootDigits], raw);
        }
        ok = hipMemcpyAsync(d_roots_raw, roots_raw.data(), roots_raw.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(f.roots, digits.data(), digits.size(), hipMemcpyHostToDevice, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;   // (the host vectors leave scope)
    }
    if (ok) {
        WsUse wsu(c, st);
        for (size_t off = 0; off < (size_t)kFk20Bases; off += kMaxChunk) {
            launch_fk20_base_rows(c->ws.scalars, d_roots_raw, (uint32_t)off, kMaxChunk, st);
            msm_stages(c, c->ws.scalars, d_comp + 48 * off, kMaxChunk, st);   // over the monomial form, on whatever engine it has
        }
        launch_g1_decompress(d_comp, f.bases, d_status, kFk20Bases, 0, st);   // (our own sums: in the subgroup by construction)
        ok = hipMemcpyAsync(h_status.data(), d_status, (size_t)kFk20Bases * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
        for (int i = 0; ok && i < kFk20Bases; i++)
            if (h_status[i] != 0) ok = false, at_infinity = true;
        if (ok) {
            launch_fk20_table(f.bases, f.table, bits, st);
            ok = hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
        }
    }
    if (d_comp) hipFree(d_comp);
    if (d_status) hipFree(d_status);
    if (d_roots_raw) hipFree(d_roots_raw);
    if (!ok) {
        (void)hipGetLastError();   // an out-of-memory here is an answer, not a sticky failure
        const size_t bytes = f.table_bytes;
        state_free(f);
        if (at_infinity) set_error("lwkzg_set_cell_proof_engine: a transformed base of this setup is the point at infinity: the engine stays as it was");
        else set_error("lwkzg_set_cell_proof_engine: the FK20 table of %d bits (%zu bytes) and its scratch could not be had: the engine stays as it was", bits, bytes);
        return C_KZG_MALLOC;
    }
    f.bits = bits;
    return C_KZG_OK;
}

void point_record(uint8_t *out, bool inf, const uint8_t *xy96) {
    out[0] = inf ? 1 : 0;
    if (inf) memset(out + 1, 0, 96);
    else memcpy(out + 1, xy96, 96);
}

C_KZG_RET fk20_points_impl(uint8_t *out, int what, const Blob *blob, const KZGSettings *s) {
    if (!s) return C_KZG_BADARGS;
    if (!out || what < 0 || what > 2 || (what != 0 && !blob)) {
        set_error("lwkzg_fk20_points: no output, no blob, or `what` is not 0, 1 or 2");
        return C_KZG_BADARGS;
    }
    const int mode = mode_of(s);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    c = c->primary;
    std::lock_guard<std::mutex> lk(c->mu);
    Fk20State &f = c->fk20;
    if (f.engine != LWKZG_CELL_PROOFS_FK20) {
        set_error("lwkzg_fk20_points: the settings' cell proof engine is not FK20");
        return C_KZG_ERROR;
    }
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (what == 0) {
        std::vector<G1Affine> h((size_t)kFk20Bases);
        LWK_HIP(hipMemcpyAsync(h.data(), f.bases, h.size() * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
        LWK_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < kFk20Bases; b++) {
            uint32_t raw[12];
            uint8_t xy[96];
            fe_to_raw<FpParams>(raw, h[b].x);
            raw_to_be<12>(xy, raw);
            fe_to_raw<FpParams>(raw, h[b].y);
            raw_to_be<12>(xy + 48, raw);
            point_record(out + 97 * (size_t)b, false, xy);   // never infinity: state_build refuses a setup with such a base
        }
        return C_KZG_OK;
    }
    G1Xyzz29 *e_copy = f.hook_pts, *h_out = f.hook_pts + kFk20Points;
    uint8_t *d_xy = (uint8_t *)(f.hook_pts + kHookPoints);
    int32_t *d_inf = (int32_t *)(d_xy + (size_t)kFk20Points * 96);
    const size_t n_pts = what == 1 ? kFk20Points : kFk20Terms;
    std::vector<uint8_t> xy(n_pts * 96);
    std::vector<int32_t> inf(n_pts);
    int32_t status = 0;
    {
        WsUse wsu(c, st);
        Workspace &w = c->ws;
        LWK_HIP(hipMemcpyAsync(w.blobs, blob, kBlobBytes, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemsetAsync(w.status, 0, 4, st));
        if (!mode_rules(mode).evaluation_form) launch_parse_be_reduce(w.blobs, w.scalars, kBlobElems, st);
        else launch_blob_evaluations_to_coefficients(w.blobs, w.scalars, c->tw28_inv, w.status, 1, st, mode_rules(mode).le());
        LWK_HIP(fk20_proofs(c, nullptr, 1, st, e_copy, h_out));
        launch_xyzz29_to_affine_be(what == 1 ? e_copy : h_out, d_xy, d_inf, n_pts, st);
        LWK_HIP(hipMemcpyAsync(xy.data(), d_xy, xy.size(), hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(inf.data(), d_inf, n_pts * 4, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(&status, w.status, 4, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipStreamSynchronize(st));
        LWK_HIP(hipGetLastError());
    }
    if (status != 0) {
        set_error("lwkzg_fk20_points: blob rejected (status %d)", status);
        return map_rc((C_KZG_RET)status, mode);
    }
    for (size_t k = 0; k < n_pts; k++) {
        size_t at = k;   // E[m] lies at position rev7(m)
        if (what == 1) {
            at = 0;
            for (int b = 0; b < 7; b++) at |= ((k >> b) & 1u) << (6 - b);
        }
        point_record(out + 97 * k, inf[at] != 0, &xy[96 * at]);
    }
    return C_KZG_OK;
}

}  // namespace

void fk20_free(Ctx *c) { state_free(c->fk20); }

hipError_t fk20_proofs(Ctx *c, uint8_t *proofs48, size_t m, hipStream_t st, G1Xyzz29 *e_copy, G1Xyzz29 *h_out) {
    const Fk20State &f = c->fk20;
    Workspace &w = c->ws;
    launch_fk20_coeffs(w.scalars, c->tw_fwd, w.scalars2, m, st);
    launch_fk20_msm(f.table, f.bits, w.scalars2, f.pts, m, st);
    hipError_t e = hipSuccess;
    if (e_copy) e = hipMemcpyAsync(e_copy, f.pts, (size_t)kFk20Points * sizeof(G1Xyzz29), hipMemcpyDeviceToDevice, st);
    launch_fk20_transforms(f.pts, f.roots, h_out, m, st);
    if (proofs48) launch_finalize_compress(f.pts, proofs48, m * kFk20Points, st);
    return e;
}

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_set_cell_proof_engine(const KZGSettings *s, int engine, int window_bits, size_t min_blobs) {
    return guarded("lwkzg_set_cell_proof_engine", [&]() -> C_KZG_RET {
        if (!s) return C_KZG_BADARGS;
        if (engine != LWKZG_CELL_PROOFS_MSM && engine != LWKZG_CELL_PROOFS_FK20) {
            set_error("lwkzg_set_cell_proof_engine: engine must be LWKZG_CELL_PROOFS_MSM (0) or LWKZG_CELL_PROOFS_FK20 (1), got %d", engine);
            return C_KZG_BADARGS;
        }
        const int bits = window_bits ? window_bits : kFk20DefaultBits;
        if (fk20_plan(bits).c == 0) {
            set_error("lwkzg_set_cell_proof_engine: window_bits must be 0, 4, 6, 7, 8 or 9 (got %d)", window_bits);
            return C_KZG_BADARGS;
        }
        Ctx *c = ctx_of(s);
        if (!c) return C_KZG_ERROR;
        c = c->primary;
        std::lock_guard<std::mutex> lk(c->mu);
        // the twin context launches against the same table under its own lock: keep it out as well (lock order: main, twin)
        std::unique_lock<std::mutex> lk_twin;
        Ctx *const twin = c->twin.load(std::memory_order_acquire);
        if (twin) lk_twin = std::unique_lock<std::mutex>(twin->mu);
        LWK_HIP(hipSetDevice(c->device));
        LWK_HIP(hipDeviceSynchronize());   // the table may be in use on any stream, the callers' included
        Fk20State &f = c->fk20;
        if (engine == LWKZG_CELL_PROOFS_MSM) {
            state_free(f);
            sync_twin(c);
            return C_KZG_OK;
        }
        const size_t from = min_blobs ? min_blobs : (size_t)LWKZG_FK20_DEFAULT_MIN_BLOBS;
        if (f.engine == LWKZG_CELL_PROOFS_FK20 && f.bits == bits) {
            f.min_blobs = from;
            sync_twin(c);
            return C_KZG_OK;
        }
        Fk20State next;   // the old table stays until the new one stands: a failure leaves the engine as it was
        const C_KZG_RET rc = state_build(c, next, bits);
        if (rc != C_KZG_OK) return rc;
        state_free(f);
        f = next;
        f.engine = LWKZG_CELL_PROOFS_FK20;
        f.min_blobs = from;
        sync_twin(c);
        return C_KZG_OK;
    });
}

int lwkzg_cell_proof_engine(const KZGSettings *s) {
    if (!s) return -1;
    Ctx *c = ctx_of(s);
    if (!c) return -1;
    c = c->primary;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->fk20.engine;
}

size_t lwkzg_fk20_table_bytes(const KZGSettings *s) {
    if (!s) return 0;
    Ctx *c = ctx_of(s);
    if (!c) return 0;
    c = c->primary;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->fk20.table ? c->fk20.table_bytes : 0;
}

size_t lwkzg_fk20_chunk_blobs(void) { return kFk20ChunkBlobs; }

C_KZG_RET lwkzg_fk20_points(uint8_t *out, int what, const Blob *blob, const KZGSettings *s) {
    return guarded("lwkzg_fk20_points", [&] { return fk20_points_impl(out, what, blob, s); });
}

}  // extern "C"
