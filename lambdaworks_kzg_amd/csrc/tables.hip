// tables.hip -- the two forms of the setup (monomial, Lagrange) and the direct tables over them: derivation of the Lagrange form, table
// builds, the moves a mode switch asks for, and the lwkzg_enable_direct_table* / lwkzg_direct_* entry points.
#include "engine_internal.h"
#include "abi_guard.h"
#include "setup_text.h"

#include <chrono>
#include <vector>

namespace lwk {

// ---- the two forms of the setup and their direct tables --------------------------------------------------------------------------
//
// A settings object has its MSM tables in up to two forms: monomial ([tau^i]G: what reference mode commits over, and what a
// quotient in coefficient form needs) and Lagrange ([l_i(tau)]G: what a c-kzg blob's evaluations commit over with no transform).
// The 9 MB bucket tables exist in both forms as soon as c-kzg mode is first used; the DIRECT table (7 .. 275 GB) is built
//   * in the form of the mode the settings answer in when it is built (lwkzg_enable_direct_table, the load's own choice) or are
//     switched to (lwkzg_settings_set_mode) -- the primary form --,
//   * and in the other form too whenever that fits beside it with kDirectAlignedHeadroom to spare (always up to 14 bits on an empty
//     MI355X; never at 15 / 16 bits) and is of use (the Lagrange form only once c-kzg mode has been used).
// A call never depends on which exist: a c-kzg commitment takes the Lagrange table when there is one, else the transform and the
// monomial table, else Lagrange buckets; a proof's quotient (coefficient form) takes the monomial table when there is one, else one
// forward transform and the Lagrange table; reference mode on a Lagrange-only table falls back to the monomial buckets.

// the twin context holds copies of every table address: refresh them (caller holds both contexts' locks)
static void sync_twin_tables(Ctx *c) {
    Ctx *t = c->twin.load(std::memory_order_acquire);
    if (!t) return;
    t->direct_table = c->direct_table;
    t->direct_tab.win_dev = c->direct_tab.win_dev;
    t->direct_bits = c->direct_bits;
    t->direct_row_bytes = c->direct_row_bytes;
    t->lag = c->lag;
    t->lag.direct_tab = DirectTable();
    t->lag.direct_tab.win_dev = c->lag.direct_tab.win_dev;
    t->lag_ready.store(c->lag.ready, std::memory_order_release);
    t->fk20 = c->fk20;   // (the FK20 engine's table and scratch: fk20_api.hip)
}

struct FormRef {  // one form's direct-table fields
    const G1Affine *points;
    DirectTable &tab;
    G1Affine29 *&table0;
    int &bits;
    size_t &row;
};
static FormRef form_ref(Ctx *c, bool lagrange) {
    if (lagrange) return {c->lag.points, c->lag.direct_tab, c->lag.direct_table, c->lag.direct_bits, c->lag.direct_row_bytes};
    return {c->points, c->direct_tab, c->direct_table, c->direct_bits, c->direct_row_bytes};
}
static void form_drop(Ctx *c, bool lagrange) {
    FormRef f = form_ref(c, lagrange);
    free_direct_table(f.tab);
    f.table0 = nullptr;
    f.bits = 0;
}

// one form's direct table of `bits`: rows aligned to 128-byte lines when that table leaves kDirectAlignedHeadroom of HBM free
// (workspaces, the caller's own buffers), packed otherwise; LWKZG_DIRECT_ROW=112|128 or row_pref forces one (A/B runs).
// need_headroom: 1 = build only if even the packed table leaves the headroom (a secondary form somebody asked for must not crowd the
// device); 2 = only if it takes at most a quarter of what is free now (the rule the load picks its own table by: a second table
// nobody asked for -- the first c-kzg call of a settings object that follows the process default -- gets no more than the first did).
static hipError_t form_build(Ctx *c, bool lagrange, int bits, size_t row_pref, int need_headroom, BuildTiming &bt) {
    FormRef f = form_ref(c, lagrange);
    auto build_rows = [&](size_t row) -> hipError_t {
        double ms[4] = {0, 0, 0, 0};
        const hipError_t e = build_direct_table(bits, f.points, f.tab, row, c->stream, ms);
        bt.scratch_malloc_ms += ms[0];
        bt.table_malloc_ms += ms[1];
        bt.kernels_ms += ms[2];
        bt.scratch_free_ms += ms[3];
        if (e != hipSuccess) {
            (void)hipGetLastError();  // an out-of-memory here is an answer, not a sticky failure
            return e;
        }
        f.table0 = (G1Affine29 *)f.tab.win[0];
        f.bits = bits;
        f.row = row;
        bt.bits = bits;
        bt.row_bytes = row;
        bt.table_bytes += direct_table_entries(bits) * row;
        return hipSuccess;
    };
    const int forced_env = knobs().direct_row;
    const int forced = forced_env ? forced_env : (int)row_pref;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) (void)hipGetLastError();
    if (need_headroom && direct_table_entries(bits) * kDirectRowPacked + kDirectAlignedHeadroom > free_b) return hipErrorOutOfMemory;
    if (need_headroom == 2 && direct_table_entries(bits) * kDirectRowPacked > free_b / 4) return hipErrorOutOfMemory;
    const bool aligned_fits = direct_table_entries(bits) * kDirectRowAligned + kDirectAlignedHeadroom <= free_b;
    if (forced == (int)kDirectRowAligned || (forced != (int)kDirectRowPacked && aligned_fits))
        if (build_rows(kDirectRowAligned) == hipSuccess) return hipSuccess;
    return build_rows(kDirectRowPacked);
}

// The Lagrange form of the setup, derived on the device: the 4096 rows of inverse-DFT coefficients (k_idft_columns) committed by
// the monomial engine as it stands, the results decompressed into affine points, the bucket engine's table built over them.
// About 50 ms on the default engine. Caller holds the primary context's lock and its twin's.
static C_KZG_RET lagrange_prepare(Ctx *c) {
    if (c->lag.ready) return C_KZG_OK;
    if (c->lag_failed) return C_KZG_MALLOC;
    LWK_HIP(hipSetDevice(c->device));
    C_KZG_RET rc = ctx_reserve(c, kMaxChunk);
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    hipStream_t st = c->stream;
    WsUse wsu(c, st);
    uint8_t *d_comp = nullptr;
    int32_t *d_status = nullptr;
    bool ok = hipMalloc((void **)&c->lag.points, (size_t)kBlobElems * sizeof(G1Affine)) == hipSuccess &&
              hipMalloc((void **)&c->lag.table, (size_t)kTablePoints * sizeof(G1Affine29)) == hipSuccess &&
              hipMalloc((void **)&d_comp, (size_t)kBlobElems * 48) == hipSuccess && hipMalloc((void **)&d_status, (size_t)kBlobElems * 4) == hipSuccess;
    std::vector<int32_t> h_status(kBlobElems, 0);
    if (ok) {
        for (size_t off = 0; off < (size_t)kBlobElems; off += kMaxChunk) {
            launch_idft_columns(w.scalars, c->tw_inv, (uint32_t)off, kMaxChunk, st);
            msm_stages(c, w.scalars, d_comp + 48 * off, kMaxChunk, st);   // over the monomial form, on whatever engine it has
        }
        launch_g1_decompress(d_comp, c->lag.points, d_status, kBlobElems, 0, st);  // (our own sums: in the subgroup by construction)
        launch_build_table(c->lag.points, c->lag.table, st);
        ok = hipMemcpyAsync(h_status.data(), d_status, (size_t)kBlobElems * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (d_comp) hipFree(d_comp);
    if (d_status) hipFree(d_status);
    for (int i = 0; ok && i < kBlobElems; i++)
        if (h_status[i] != 0) ok = false;  // (an l_i(tau) G at infinity: tau would have to be a root of l_i, i.e. a domain point)
    if (!ok) {
        (void)hipGetLastError();
        dev_free(c->lag.points);
        dev_free(c->lag.table);
        c->lag_failed = true;
        set_error("the Lagrange form of the setup could not be derived (out of device memory, or tau is a 4096th root of unity): c-kzg mode stays on the transform");
        return C_KZG_MALLOC;
    }
    c->lag.ready = true;
    c->lag_ready.store(true, std::memory_order_release);
    return C_KZG_OK;
}

// ---- a setup that arrives in Lagrange form (load.hip: the c-kzg loaders) ---------------------------------------------------------
// The context is the loader's own until the load returns: no lock is taken here. Everything is enqueued on the context's stream; the
// loader reads the verdicts and decides.
C_KZG_RET lagrange_from_bytes(Ctx *c, const uint8_t *d_in48, int32_t *d_status) {
    if (hipMalloc((void **)&c->lag.points, (size_t)kBlobElems * sizeof(G1Affine)) != hipSuccess ||
        hipMalloc((void **)&c->lag.table, (size_t)kTablePoints * sizeof(G1Affine29)) != hipSuccess) {
        (void)hipGetLastError();
        dev_free(c->lag.points);
        dev_free(c->lag.table);
        set_error("hipMalloc failed for the Lagrange form of the setup");
        return C_KZG_MALLOC;
    }
    launch_g1_decompress(d_in48, c->lag.points, d_status, kBlobElems, 1, c->stream);
    launch_build_table(c->lag.points, c->lag.table, c->stream);
    return C_KZG_OK;
}

// [tau^j]G = sum_k w_k^j L_k (fr_ops.hip: k_dft_rows): lagrange_prepare the other way round, the same 4096 MSMs over the other form.
// The Lagrange form has only its bucket table at this point of a load, so that is the engine they run on.
C_KZG_RET monomial_from_lagrange(Ctx *c, uint8_t *d_comp48) {
    C_KZG_RET rc = ctx_reserve(c, kMaxChunk);
    if (rc != C_KZG_OK) return rc;
    hipStream_t st = c->stream;
    WsUse wsu(c, st);
    for (size_t off = 0; off < (size_t)kBlobElems; off += kMaxChunk) {
        launch_dft_rows(c->ws.scalars, c->tw_fwd, (uint32_t)off, kMaxChunk, st);
        msm_stages(c, c->ws.scalars, d_comp48 + 48 * off, kMaxChunk, st, 0, false, true);
    }
    return C_KZG_OK;
}

void lagrange_publish(Ctx *c) {
    c->lag.ready = true;
    c->lag_ready.store(true, std::memory_order_release);
}

C_KZG_RET lagrange_ensure(Ctx *c) {
    c = c->primary;
    if (c->lag_ready.load(std::memory_order_acquire)) return C_KZG_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    std::unique_lock<std::mutex> lk_twin;
    Ctx *const twin = c->twin.load(std::memory_order_acquire);
    if (twin) lk_twin = std::unique_lock<std::mutex>(twin->mu);
    LWK_HIP(hipSetDevice(c->device));
    LWK_HIP(hipDeviceSynchronize());
    c->lag_failed = false;   // (an explicit request retries, as lwkzg_settings_set_mode does)
    const C_KZG_RET rc = lagrange_prepare(c);
    hipDeviceSynchronize();
    sync_twin_tables(c);
    return rc;
}

// Bring the tables to what mode `mode` wants (see the block comment above). `may_swap`: when the mode's form has no direct table,
// the other has one and the two do not fit side by side, move the table over (explicit requests: lwkzg_settings_set_mode,
// lwkzg_enable_direct_table); lazily (first c-kzg call of a settings object that follows the process-wide default) only the
// free-of-charge secondary build is tried. Caller holds the primary context's lock and its twin's; the device is idle.
static void tables_follow_mode(Ctx *c, int mode, bool may_swap) {
    const bool want_lag = mode_rules(mode).evaluation_form;   // (c-kzg and eth mode alike: moving between the two moves nothing)
    if (want_lag && lagrange_prepare(c) != C_KZG_OK) return;
    const int bits = c->direct_bits ? c->direct_bits : c->lag.direct_bits;
    if (!bits) return;                                     // bucket engine: both forms have their 9 MB tables
    FormRef mine = form_ref(c, want_lag);
    if (mine.bits == bits) return;
    BuildTiming bt;
    if (form_build(c, want_lag, bits, 0, may_swap ? 1 : 2, bt) == hipSuccess) return;  // fits beside the other: both forms live
    if (!may_swap) return;
    // The two forms' tables have the SAME geometry (width, windows, row size): the other form's allocations move over as they are and
    // the build kernels run again over them -- no hipFree / hipMalloc of 275 GB, no wait for the driver's scrub (7-8.5 s ->
    // the kernels' half second). LWKZG_SET_MODE_IN_PLACE=0: free and allocate, the A/B arm.
    const bool in_place_on = knobs().set_mode_in_place;
    FormRef other = form_ref(c, !want_lag);
    if (in_place_on && other.bits == bits && other.table0) {
        auto wall = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t0 = wall();
        const size_t row = other.row;
        mine.tab = other.tab;
        other.tab = DirectTable();
        other.table0 = nullptr;
        other.bits = 0;
        double ms[4] = {0, 0, 0, 0};
        if (build_direct_table(bits, mine.points, mine.tab, row, c->stream, ms, true) == hipSuccess) {
            mine.table0 = (G1Affine29 *)mine.tab.win[0];
            mine.bits = bits;
            mine.row = row;
            bt.bits = bits;
            bt.row_bytes = row;
            bt.table_bytes = direct_table_entries(bits) * row;
            bt.scratch_malloc_ms = ms[0];
            bt.kernels_ms = ms[2];
            bt.scratch_free_ms = ms[3];
            bt.total_ms = wall() - t0;
            bt.in_place = true;
            c->last_build = bt;
            return;
        }
        (void)hipGetLastError();   // (the failed build freed what it held: fall through to a build from nothing)
        mine.table0 = nullptr;
        mine.bits = 0;
    } else {
        form_drop(c, !want_lag);
    }
    if (form_build(c, want_lag, bits, 0, 0, bt) != hipSuccess) (void)form_build(c, !want_lag, bits, 0, 0, bt);  // (cannot happen: the other form's table just left)
    c->last_build = bt;
}

// Called by every compute entry point before it takes its context: a settings object answering in c-kzg mode gets the Lagrange form
// on first use (and a Lagrange direct table if one fits beside the monomial one). One atomic load afterwards.
void ensure_lagrange(Ctx *c, int mode) {
    if (!mode_rules(mode).evaluation_form || c->lag_ready.load(std::memory_order_acquire)) return;
    c = c->primary;
    std::lock_guard<std::mutex> lk(c->mu);
    std::unique_lock<std::mutex> lk_twin;
    Ctx *const twin = c->twin.load(std::memory_order_acquire);
    if (twin) lk_twin = std::unique_lock<std::mutex>(twin->mu);
    if (c->lag.ready || c->lag_failed) return;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return;
    tables_follow_mode(c, mode, false);
    hipDeviceSynchronize();
    sync_twin_tables(c);
}

void settings_follow_mode(Ctx *c, int mode) {
    c = c->primary;
    std::lock_guard<std::mutex> lk(c->mu);
    std::unique_lock<std::mutex> lk_twin;
    Ctx *const twin = c->twin.load(std::memory_order_acquire);
    if (twin) lk_twin = std::unique_lock<std::mutex>(twin->mu);
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return;
    c->lag_failed = false;   // an explicit request retries a derivation that once ran out of memory (only the lazy path stays off: ADVICE r04)
    tables_follow_mode(c, mode, true);
    hipDeviceSynchronize();
    sync_twin_tables(c);
}

// row_pref: 0 = rows aligned to 128-byte lines when that leaves headroom on the device, else packed; or one of the two
// forms: 0 = by the settings' mode (the rule above); 1 / 2 / 3 = exactly the monomial / the Lagrange / both forms (lwkzg_enable_direct_table_forms)
C_KZG_RET enable_direct_table(const KZGSettings *s, int window_bits, size_t row_pref, int forms) {
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (forms < 0 || forms > 3) {
        set_error("lwkzg_enable_direct_table_forms: forms must be 1 (monomial), 2 (Lagrange) or 3 (both)");
        return C_KZG_BADARGS;
    }
    const bool want_lag = forms == 2 || forms == 3 ? true : forms == 1 ? false : mode_rules(mode_of(s)).evaluation_form;
    std::lock_guard<std::mutex> lk(c->mu);
    // the twin context launches against the same table under its own lock: keep it out as well (lock order: main, twin)
    std::unique_lock<std::mutex> lk_twin;
    Ctx *const twin = c->twin.load(std::memory_order_acquire);
    if (twin) lk_twin = std::unique_lock<std::mutex>(twin->mu);
    LWK_HIP(hipSetDevice(c->device));
    LWK_HIP(hipDeviceSynchronize());  // the table may be in use on any stream, the callers' included
    const int old_bits = c->direct_bits ? c->direct_bits : c->lag.direct_bits;
    const int old_forms = (c->direct_table ? 1 : 0) | (c->lag.direct_table ? 2 : 0);
    if (window_bits == old_bits && (forms == 0 || forms == old_forms || window_bits == 0)) return C_KZG_OK;
    if (window_bits != 0 && direct_table_entries(window_bits) == 0) {
        set_error("lwkzg_enable_direct_table: window_bits must be 0 or 10 .. 16 (got %d)", window_bits);
        return C_KZG_BADARGS;
    }
    auto wall = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = wall();
    // the primary form: the one the settings' mode commits over (Lagrange only if it can be had)
    c->lag_failed = false;   // (an explicit request retries a derivation that once ran out of memory)
    const bool primary_lag = want_lag && lagrange_prepare(c) == C_KZG_OK;
    if (forms >= 2 && !primary_lag) return C_KZG_MALLOC;  // (lagrange_prepare has said why)
    form_drop(c, false);  // (the old and the new tables need not fit side by side)
    form_drop(c, true);
    BuildTiming bt;
    bt.free_old_ms = wall() - t_start;
    sync_twin_tables(c);
    if (window_bits == 0) return C_KZG_OK;
    hipError_t e = form_build(c, primary_lag, window_bits, row_pref, 0, bt);
    if (e == hipSuccess && forms == 3) e = form_build(c, false, window_bits, row_pref, 0, bt);
    if (e == hipSuccess && forms == 0 && (primary_lag || c->lag.ready)) (void)form_build(c, !primary_lag, window_bits, row_pref, 1, bt);  // the other form, if it fits beside
    if (e != hipSuccess) {
        form_drop(c, false);
        form_drop(c, true);
    }
    bt.total_ms = wall() - t_start;
    c->last_build = bt;
    if (e != hipSuccess) {
        if (old_bits) {  // the engine the settings had stays in place (the form it was in first)
            BuildTiming scratch;
            const bool first_lag = old_forms == 2 || (old_forms == 3 && primary_lag);
            if (form_build(c, first_lag, old_bits, row_pref, 0, scratch) == hipSuccess && old_forms == 3)
                (void)form_build(c, !first_lag, old_bits, row_pref, 1, scratch);
        }
        sync_twin_tables(c);
        set_error("lwkzg_enable_direct_table(%d): %zu bytes: %s", window_bits, direct_table_entries(window_bits) * kDirectRowPacked,
                  hipGetErrorString(e));
        return C_KZG_MALLOC;
    }
    sync_twin_tables(c);
    return C_KZG_OK;
}

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_enable_direct_table(const KZGSettings *s, int window_bits) { return enable_direct_table(s, window_bits, 0); }
C_KZG_RET lwkzg_enable_direct_table_forms(const KZGSettings *s, int window_bits, int forms) {
    if (forms < 1 || forms > 3) {
        set_error("lwkzg_enable_direct_table_forms: forms must be 1 (monomial), 2 (Lagrange) or 3 (both)");
        return C_KZG_BADARGS;
    }
    return enable_direct_table(s, window_bits, 0, forms);
}

int lwkzg_direct_table_bits(const KZGSettings *s) {
    Ctx *c = ctx_of(s);
    return !c ? -1 : c->direct_bits ? c->direct_bits : c->lag.direct_bits;
}

// bit 0: a direct table over the monomial form is live; bit 1: one over the Lagrange form (c-kzg mode without the transform)
int lwkzg_direct_table_forms(const KZGSettings *s) {
    Ctx *c = ctx_of(s);
    return !c ? -1 : (c->direct_table ? 1 : 0) | (c->lag.direct_table ? 2 : 0);
}

// The Lagrange form of a loaded setup as a c-kzg-4844 1.x file holds it: 4096 x 48 bytes compressed, NATURAL order. Derived first if the
// settings have not needed it yet (C_KZG_MALLOC, as lwkzg_settings_set_mode's derivation, when it cannot be had).
C_KZG_RET lwkzg_setup_g1_lagrange(uint8_t *out, const KZGSettings *s) {
    if (!out || !s) return C_KZG_BADARGS;
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_BADARGS;
    return guarded("lwkzg_setup_g1_lagrange", [&]() -> C_KZG_RET {
        C_KZG_RET rc = lagrange_ensure(c);
        if (rc != C_KZG_OK) return rc;
        Ctx *p = c->primary;
        std::vector<G1Affine> pts(kBlobElems);
        std::vector<uint8_t> comp((size_t)kBlobElems * 48);
        {
            std::lock_guard<std::mutex> lk(p->mu);
            LWK_HIP(hipSetDevice(p->device));
            LWK_HIP(hipMemcpyAsync(pts.data(), p->lag.points, (size_t)kBlobElems * sizeof(G1Affine), hipMemcpyDeviceToHost, p->stream));
            LWK_HIP(hipStreamSynchronize(p->stream));
        }
        for (size_t i = 0; i < (size_t)kBlobElems; i++) g1_compress_affine(&comp[48 * i], pts[i]);   // (never the point at infinity: lagrange_prepare, the loaders)
        setup_text_bitrev48(out, comp.data());   // the library's order is the blob's own; a c-kzg file's is the natural one
        return C_KZG_OK;
    });
}

int lwkzg_direct_num_windows(int window_bits) { return direct_num_windows(window_bits); }

int lwkzg_direct_row_bytes(const KZGSettings *s) {
    Ctx *c = ctx_of(s);
    return !c ? -1 : c->direct_table ? (int)c->direct_row_bytes : c->lag.direct_table ? (int)c->lag.direct_row_bytes : 0;
}

}  // extern "C"
