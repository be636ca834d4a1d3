// load.hip -- a trusted setup's way in and out: load from bytes or a file, free, release of a cached context, and the device image that
// hands a loaded setup to another GPU.
#include "engine_internal.h"
#include "abi_guard.h"
#include "fp2.h"
#include "setup_text.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

namespace lwk {
bool pairing_product_is_one_uncached(const G1Affine *ps, const Fp2 *qx, const Fp2 *qy, int n);   // pairing.hip
}
using namespace lwk;

extern "C" {

// ------------------------------------------------------------------------------------------------
// trusted setup

static C_KZG_RET setup_from_bytes(KZGSettings *out, const uint8_t *g1_bytes, const uint8_t *g2_bytes) {
    Ctx *c = nullptr;
    auto wall = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = wall();
    C_KZG_RET rc = ctx_new(&c);
    if (rc != C_KZG_OK) return rc;
    LoadTiming lt;
    lt.context_ms = wall() - t_start;
    double t_mark = wall();
    const size_t n1 = kBlobElems, n2 = TRUSTED_SETUP_NUM_G2_POINTS;
    uint8_t *d_in = nullptr;
    int32_t *d_status = nullptr;
    uint64_t *d_blst = nullptr;
    g1_t *g1v = (g1_t *)malloc(n1 * sizeof(g1_t));  // libc malloc: the reference frees these with libc::free (lib.rs:824-826)
    g2_t *g2v = (g2_t *)malloc(n2 * sizeof(g2_t));
    std::vector<int32_t> h_status(n1);
    rc = C_KZG_ERROR;
    do {
        if (!g1v || !g2v) { rc = C_KZG_MALLOC; break; }
        if (hipMalloc((void **)&d_in, n1 * 48) != hipSuccess || hipMalloc((void **)&d_status, n1 * 4) != hipSuccess ||
            hipMalloc((void **)&d_blst, n1 * 144) != hipSuccess) { rc = C_KZG_MALLOC; set_error("hipMalloc failed in setup load"); break; }
        if (hipMemcpyAsync(d_in, g1_bytes, n1 * 48, hipMemcpyHostToDevice, c->stream) != hipSuccess) { set_error("H2D of g1 bytes failed"); break; }
        // decompress_g1_point incl. the [r]P subgroup check for every point (compression.rs:62-103)
        launch_g1_decompress(d_in, c->points, d_status, n1, 1, c->stream);
        launch_g1_to_blst(c->points, d_status, d_blst, n1, c->stream);
        launch_build_table(c->points, c->table, c->stream);
        if (hipMemcpyAsync(h_status.data(), d_status, n1 * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(g1v, d_blst, n1 * 144, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { set_error("setup kernels failed: %s", hipGetErrorString(hipGetLastError())); break; }
        bool good = true;
        for (size_t i = 0; i < n1; i++) {
            if (h_status[i] == 2) { set_error("g1 point %zu: invalid compressed point or not in the subgroup", i); good = false; break; }
            if (h_status[i] == 1) { set_error("g1 point %zu is the point at infinity: the reference cannot read such a setup back (srs.rs:155-172)", i); good = false; break; }
        }
        if (!good) break;
        lt.points_and_tables_ms = wall() - t_mark;
        t_mark = wall();
        if (!g2_fill_values(g2v, g2_bytes, n2)) { if (!get_error()[0]) set_error("invalid g2 point in trusted setup"); break; }
        rc = ctx_finish_fft(c);
        lt.g2_and_fft_ms = wall() - t_mark;
    } while (0);
    if (d_in) hipFree(d_in);
    if (d_status) hipFree(d_status);
    if (d_blst) hipFree(d_blst);
    if (rc != C_KZG_OK) {
        free(g1v);
        free(g2v);
        ctx_destroy(c);
        return rc;
    }
    out->fs = &c->fs;
    out->g1_values = g1v;
    out->g2_values = g2v;
    t_mark = wall();
    direct_from_env(out);
    lt.default_table_ms = wall() - t_mark;
    lt.total_ms = wall() - t_start;
    c->load_timing = lt;
    return C_KZG_OK;
}

C_KZG_RET load_trusted_setup(KZGSettings *out, const uint8_t *g1_bytes, size_t n1, const uint8_t *g2_bytes, size_t n2) {
    if (!out || !g1_bytes || !g2_bytes) return C_KZG_BADARGS;
    if (n1 != TRUSTED_SETUP_NUM_G1_POINTS || n2 != TRUSTED_SETUP_NUM_G2_POINTS) return C_KZG_BADARGS;  // lib.rs:716-718
    return setup_from_bytes(out, g1_bytes, g2_bytes);
}

static int hexv(int ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    if (ch >= 'A' && ch <= 'F') return ch - 'A' + 10;
    return -1;
}

// srs.rs:25-82: line 1 = n1, line 2 = n2 (decimal), then exactly one hex point per line.
C_KZG_RET load_trusted_setup_file(KZGSettings *out, FILE *in) {
    if (!out || !in) return C_KZG_BADARGS;
    std::string text;
    char buf[64 * 1024];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, in)) > 0) text.append(buf, got);  // lib.rs:780-789
    std::vector<std::pair<size_t, size_t>> lines;  // (offset, length), str::lines semantics
    size_t pos = 0;
    while (pos < text.size()) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        size_t len = e - pos;
        if (len && text[pos + len - 1] == '\r') len--;
        lines.push_back({pos, len});
        pos = e + 1;
    }
    auto parse_count = [&](size_t li, size_t *v) -> bool {
        if (li >= lines.size()) return false;
        size_t o = lines[li].first, l = lines[li].second, k = 0;
        if (l && text[o] == '+') k = 1;
        if (k == l) return false;
        size_t acc = 0;
        for (; k < l; k++) {
            char ch = text[o + k];
            if (ch < '0' || ch > '9') return false;
            acc = acc * 10 + (size_t)(ch - '0');
            if (acc > (1u << 24)) return false;
        }
        *v = acc;
        return true;
    };
    size_t n1 = 0, n2 = 0;
    if (!parse_count(0, &n1) || !parse_count(1, &n2)) {
        set_error("trusted setup file: bad header");
        return C_KZG_ERROR;
    }
    // The reference does not check n1 here and later reads 4096 entries regardless (UB for other
    // sizes); this engine is built for 4096/65 and says so.
    if (n1 != TRUSTED_SETUP_NUM_G1_POINTS || n2 != TRUSTED_SETUP_NUM_G2_POINTS) {
        set_error("trusted setup file announces %zu/%zu points; this engine needs 4096/65", n1, n2);
        return C_KZG_BADARGS;
    }
    if (lines.size() < 2 + n1 + n2) {
        set_error("trusted setup file: %zu point lines, expected %zu", lines.size() - 2, n1 + n2);
        return C_KZG_ERROR;
    }
    std::vector<uint8_t> g1(n1 * 48), g2(n2 * 96);
    for (size_t i = 0; i < n1 + n2; i++) {
        size_t nb = i < n1 ? 48 : 96;
        uint8_t *dst = i < n1 ? &g1[i * 48] : &g2[(i - n1) * 96];
        size_t o = lines[2 + i].first, l = lines[2 + i].second;
        if (l != 2 * nb) {
            set_error("trusted setup file: line %zu has %zu characters, expected %zu", i + 3, l, 2 * nb);
            return C_KZG_ERROR;
        }
        for (size_t k = 0; k < nb; k++) {
            int h = hexv(text[o + 2 * k]), lo = hexv(text[o + 2 * k + 1]);
            if (h < 0 || lo < 0) {
                set_error("trusted setup file: line %zu is not hex", i + 3);
                return C_KZG_ERROR;
            }
            dst[k] = (uint8_t)(h * 16 + lo);
        }
    }
    return setup_from_bytes(out, g1.data(), g2.data());
}

// ------------------------------------------------------------------------------------------------
// c-kzg-4844 trusted setups: the G1 points arrive in LAGRANGE form, natural order

static double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static size_t bitrev12(size_t i) {
    size_t r = 0;
    for (int b = 0; b < 12; b++) r |= ((i >> b) & 1u) << (11 - b);
    return r;
}
// rho^0 .. rho^(count - 1) as canonical raw scalars (8 words each) at out + 8 * first, zeros elsewhere in the 4096-scalar row
static void power_row(uint32_t *out, const Fr &rho, size_t first, size_t count) {
    memset(out, 0, (size_t)kBlobElems * 32);
    Fr cur = Fr::one();
    for (size_t j = 0; j < count; j++) {
        fe_to_raw<FrParams>(out + 8 * (first + j), cur);
        cur = cur * rho;
    }
}
static Fr fr_from_digest(const uint8_t digest[32]) {
    uint32_t raw[8];
    raw_from_be<8>(raw, digest);
    return fe_from_raw<FrParams>(raw);   // (reduces)
}

// g1_lagrange: 4096 x 48 bytes, natural order. g1_monomial: the same setup's monomial section (three-section form: both are validated
// and held against each other) or NULL (one-section form: the monomial points are derived). Every rejection of the INPUT is
// C_KZG_BADARGS, c-kzg's code, in both modes.
static C_KZG_RET setup_from_ckzg(KZGSettings *out, const uint8_t *g1_lagrange, const uint8_t *g1_monomial, const uint8_t *g2_bytes) {
    const size_t n1 = kBlobElems, n2 = TRUSTED_SETUP_NUM_G2_POINTS;
    // (host vectors first: nothing below this block throws)
    std::vector<uint8_t> permuted(n1 * 48);
    std::vector<int32_t> h_status(2 * n1);
    std::vector<uint32_t> h_rows(g1_monomial ? 2 * n1 * 8 : 0);
    setup_text_bitrev48(permuted.data(), g1_lagrange);   // the blob's own order, which the library's Lagrange form is in
    Ctx *c = nullptr;
    const double t_start = wall_ms();
    C_KZG_RET rc = ctx_new(&c);
    if (rc != C_KZG_OK) return rc;
    LoadTiming lt;
    lt.context_ms = wall_ms() - t_start;
    double t_mark = wall_ms();
    const double t_points = t_mark;
    uint8_t *d_lag = nullptr, *d_mono = nullptr, *d_pair = nullptr;
    int32_t *d_status = nullptr;   // [0, n1): the Lagrange section, [n1, 2 n1): the monomial points
    uint64_t *d_blst = nullptr;
    g1_t *g1v = (g1_t *)malloc(n1 * sizeof(g1_t));  // libc malloc, as setup_from_bytes
    g2_t *g2v = (g2_t *)malloc(n2 * sizeof(g2_t));
    hipStream_t st = c->stream;
    rc = C_KZG_ERROR;
    do {
        if (!g1v || !g2v) { rc = C_KZG_MALLOC; break; }
        if (hipMalloc((void **)&d_lag, n1 * 48) != hipSuccess || hipMalloc((void **)&d_mono, n1 * 48) != hipSuccess ||
            hipMalloc((void **)&d_pair, 96) != hipSuccess || hipMalloc((void **)&d_status, 2 * n1 * 4) != hipSuccess ||
            hipMalloc((void **)&d_blst, n1 * 144) != hipSuccess) { rc = C_KZG_MALLOC; set_error("hipMalloc failed in setup load"); break; }
        if (hipMemcpyAsync(d_lag, permuted.data(), n1 * 48, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("H2D of g1 bytes failed"); break; }
        if ((rc = lagrange_from_bytes(c, d_lag, d_status)) != C_KZG_OK) break;
        rc = C_KZG_ERROR;
        if (g1_monomial) {
            if (hipMemcpyAsync(d_mono, g1_monomial, n1 * 48, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("H2D of g1 bytes failed"); break; }
            launch_g1_decompress(d_mono, c->points, d_status + n1, n1, 1, st);
        }
        if (hipMemcpyAsync(h_status.data(), d_status, (g1_monomial ? 2 : 1) * n1 * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { set_error("setup kernels failed: %s", hipGetErrorString(hipGetLastError())); break; }
        bool good = true;
        for (size_t i = 0; i < n1 && good; i++) {   // i: the caller's (natural) index
            const int32_t v = h_status[bitrev12(i)];
            if (v == 2) { set_error("g1 lagrange point %zu: invalid compressed point or not in the subgroup", i); good = false; }
            if (v == 1) { set_error("g1 lagrange point %zu is the point at infinity", i); good = false; }
        }
        for (size_t i = 0; g1_monomial && i < n1 && good; i++) {
            if (h_status[n1 + i] == 2) { set_error("g1 monomial point %zu: invalid compressed point or not in the subgroup", i); good = false; }
            if (h_status[n1 + i] == 1) { set_error("g1 monomial point %zu is the point at infinity", i); good = false; }
        }
        if (!good) { rc = C_KZG_BADARGS; break; }
        lt.lagrange_section_ms = wall_ms() - t_mark;
        if ((rc = ctx_finish_fft(c)) != C_KZG_OK) break;   // (the rows below are written from the twiddles: they come first on this path)
        rc = C_KZG_ERROR;
        if (!g1_monomial) {
            t_mark = wall_ms();
            if ((rc = monomial_from_lagrange(c, d_mono)) != C_KZG_OK) break;
            rc = C_KZG_ERROR;
            launch_g1_decompress(d_mono, c->points, d_status + n1, n1, 0, st);  // (our own sums: in the subgroup by construction)
            if (hipMemcpyAsync(h_status.data() + n1, d_status + n1, n1 * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { set_error("setup kernels failed: %s", hipGetErrorString(hipGetLastError())); break; }
            for (size_t i = 0; i < n1 && good; i++)
                if (h_status[n1 + i] != 0) {
                    set_error("derived g1 monomial point %zu is the point at infinity: these are not the Lagrange points of a setup", i);
                    good = false;
                }
            if (!good) { rc = C_KZG_BADARGS; break; }
            lt.derive_monomial_ms = wall_ms() - t_mark;
        }
        launch_g1_to_blst(c->points, d_status + n1, d_blst, n1, st);
        launch_build_table(c->points, c->table, st);
        if (hipMemcpyAsync(g1v, d_blst, n1 * 144, hipMemcpyDeviceToHost, st) != hipSuccess) { set_error("D2H of g1_values failed"); break; }
        if (g1_monomial) {
            // the two sections against each other: p(x) = sum_j rho^j x^j committed over each -- its coefficients over the monomial points,
            // its evaluations (one forward transform, in the order the Lagrange MSM reads) over the Lagrange points
            t_mark = wall_ms();
            uint8_t digest[32], pair[96];
            sha256_fast_prefixed(digest, g1_lagrange, n1 * 48, g1_monomial, n1 * 48);
            power_row(h_rows.data(), fr_from_digest(digest), 0, n1);
            memcpy(h_rows.data() + n1 * 8, h_rows.data(), n1 * 32);
            if ((rc = ctx_reserve(c, 2)) != C_KZG_OK) break;
            rc = C_KZG_ERROR;
            {
                WsUse wsu(c, st);
                Workspace &w = c->ws;
                uint32_t *evals = w.scalars + n1 * 8;
                if (hipMemcpyAsync(w.scalars, h_rows.data(), 2 * n1 * 32, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("H2D of the cross-check scalars failed"); break; }
                launch_coefficients_to_evaluations(evals, w.fr, (Fr *)w.scalars2, c->tw28_fwd, 1, st);
                msm_stages(c, w.scalars, d_pair, 1, st, 0, false, false);
                msm_stages(c, evals, d_pair + 48, 1, st, 0, false, true);
            }
            if (hipMemcpyAsync(pair, d_pair, 96, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
                set_error("setup kernels failed: %s", hipGetErrorString(hipGetLastError()));
                break;
            }
            if (memcmp(pair, pair + 48, 48) != 0) {
                set_error("the g1 lagrange and g1 monomial sections are not the same setup (a random polynomial commits to two different points over them)");
                rc = C_KZG_BADARGS;
                break;
            }
            lt.cross_check_ms = wall_ms() - t_mark;
        } else if (hipStreamSynchronize(st) != hipSuccess) {
            set_error("setup kernels failed: %s", hipGetErrorString(hipGetLastError()));
            break;
        }
        lt.points_and_tables_ms = wall_ms() - t_points;
        t_mark = wall_ms();
        if (!g2_fill_values(g2v, g2_bytes, n2)) {
            if (!get_error()[0]) set_error("invalid g2 point in trusted setup");
            rc = C_KZG_BADARGS;
            break;
        }
        lt.g2_and_fft_ms = wall_ms() - t_mark;
        rc = C_KZG_OK;
    } while (0);
    if (rc != C_KZG_OK) (void)hipStreamSynchronize(st);   // (nothing enqueued may outlive the buffers below)
    if (d_lag) hipFree(d_lag);
    if (d_mono) hipFree(d_mono);
    if (d_pair) hipFree(d_pair);
    if (d_status) hipFree(d_status);
    if (d_blst) hipFree(d_blst);
    if (rc != C_KZG_OK) {
        (void)hipGetLastError();
        free(g1v);
        free(g2v);
        ctx_destroy(c);
        return rc;
    }
    lagrange_publish(c);
    c->mode_override.store(LWKZG_MODE_CKZG, std::memory_order_relaxed);   // before the load picks its table: that table is built in the Lagrange form first
    out->fs = &c->fs;
    out->g1_values = g1v;
    out->g2_values = g2v;
    t_mark = wall_ms();
    direct_from_env(out);
    lt.default_table_ms = wall_ms() - t_mark;
    lt.total_ms = wall_ms() - t_start;
    c->load_timing = lt;
    return C_KZG_OK;
}

C_KZG_RET lwkzg_load_trusted_setup_lagrange(KZGSettings *out, const uint8_t *g1_lagrange_bytes, size_t n1, const uint8_t *g2_bytes, size_t n2) {
    if (!out || !g1_lagrange_bytes || !g2_bytes) return C_KZG_BADARGS;
    if (n1 != TRUSTED_SETUP_NUM_G1_POINTS || n2 != TRUSTED_SETUP_NUM_G2_POINTS) {
        set_error("lwkzg_load_trusted_setup_lagrange: %zu/%zu points; this engine needs 4096/65", n1, n2);
        return C_KZG_BADARGS;
    }
    return guarded("lwkzg_load_trusted_setup_lagrange", [&] { return setup_from_ckzg(out, g1_lagrange_bytes, nullptr, g2_bytes); });
}

C_KZG_RET lwkzg_load_trusted_setup_ckzg(KZGSettings *out, const uint8_t *g1_monomial_bytes, size_t n_g1_monomial, const uint8_t *g1_lagrange_bytes,
                                        size_t n_g1_lagrange, const uint8_t *g2_monomial_bytes, size_t n_g2, uint64_t precompute) {
    (void)precompute;   // (c-kzg's own table width: this library has its tables)
    if (!out || !g1_monomial_bytes || !g1_lagrange_bytes || !g2_monomial_bytes) return C_KZG_BADARGS;
    if (n_g1_monomial != TRUSTED_SETUP_NUM_G1_POINTS || n_g1_lagrange != TRUSTED_SETUP_NUM_G1_POINTS || n_g2 != TRUSTED_SETUP_NUM_G2_POINTS) {
        set_error("lwkzg_load_trusted_setup_ckzg: %zu/%zu/%zu points; this engine needs 4096/4096/65", n_g1_monomial, n_g1_lagrange, n_g2);
        return C_KZG_BADARGS;
    }
    return guarded("lwkzg_load_trusted_setup_ckzg", [&] { return setup_from_ckzg(out, g1_lagrange_bytes, g1_monomial_bytes, g2_monomial_bytes); });
}

C_KZG_RET lwkzg_load_trusted_setup_file_ckzg(KZGSettings *out, FILE *in) {
    if (!out || !in) return C_KZG_BADARGS;
    return guarded("lwkzg_load_trusted_setup_file_ckzg", [&]() -> C_KZG_RET {
        std::string text;
        char buf[64 * 1024];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, in)) > 0) text.append(buf, got);
        SetupText t;
        if (!setup_text_parse(text.data(), text.size(), t)) {
            set_error("%s", t.error);
            return C_KZG_BADARGS;
        }
        return setup_from_ckzg(out, t.g1_lagrange.data(), t.three_sections ? t.g1_monomial.data() : nullptr, t.g2_monomial.data());
    });
}

// ------------------------------------------------------------------------------------------------
// is this a powers-of-tau setup?

static Fp fp_from_blst(const blst_fp &v) {
    uint32_t raw[12];
    for (int k = 0; k < 6; k++) {
        raw[2 * k] = (uint32_t)v.l[5 - k];
        raw[2 * k + 1] = (uint32_t)(v.l[5 - k] >> 32);
    }
    return fe_from_raw<FpParams>(raw);
}
static bool hex_bytes(uint8_t *out, const char *hex, size_t n) {
    for (size_t k = 0; k < n; k++) out[k] = (uint8_t)(hexv(hex[2 * k]) * 16 + hexv(hex[2 * k + 1]));
    return true;
}
static const char kG1GeneratorHex[] = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb";
static const char kG2GeneratorHex[] =
    "93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
    "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8";

// *ok = g1_values are [tau^i]G1 and g2_values are [tau^i]G2 for ONE tau, from the generators. Two MSMs on the settings' engine and the
// host's pairing; the settings are read, never written. What it tells apart from a setup: a Lagrange file loaded as monomial (its first
// point is not the generator, and no chain holds), any foreign, swapped or reordered point.
C_KZG_RET lwkzg_trusted_setup_check(bool *ok, const KZGSettings *s) {
    if (!ok || !s) return C_KZG_BADARGS;
    *ok = false;
    if (!s->g1_values || !s->g2_values) {
        set_error("lwkzg_trusted_setup_check: the settings hold no points");
        return C_KZG_BADARGS;
    }
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_BADARGS;
    return guarded("lwkzg_trusted_setup_check", [&]() -> C_KZG_RET {
        const size_t n1 = kBlobElems, n2 = TRUSTED_SETUP_NUM_G2_POINTS;
        // the generators
        uint8_t gen1[48], gen2[96];
        hex_bytes(gen1, kG1GeneratorHex, 48);
        hex_bytes(gen2, kG2GeneratorHex, 96);
        G1Affine g;
        g.x = Fp::zero();
        g.y = Fp::zero();
        Fp2 hx, hy;
        bool inf = false;
        if (g1_decompress_nocheck(g, gen1) != 0 || !g2_decompress(hx, hy, inf, gen2) || inf) return C_KZG_ERROR;
        G1Affine m0 = {fp_from_blst(s->g1_values[0].x), fp_from_blst(s->g1_values[0].y)};
        G1Affine m1 = {fp_from_blst(s->g1_values[1].x), fp_from_blst(s->g1_values[1].y)};
        std::vector<Fp2> qx(n2), qy(n2);
        for (size_t k = 0; k < n2; k++) {
            qx[k] = {fp_from_blst(s->g2_values[k].x.fp[0]), fp_from_blst(s->g2_values[k].x.fp[1])};
            qy[k] = {fp_from_blst(s->g2_values[k].y.fp[0]), fp_from_blst(s->g2_values[k].y.fp[1])};
        }
        if (!(m0.x == g.x) || !(m0.y == g.y) || !(qx[0].c0 == hx.c0) || !(qx[0].c1 == hx.c1) || !(qy[0].c0 == hy.c0) || !(qy[0].c1 == hy.c1))
            return C_KZG_OK;   // (verdict: false)
        // the G1 chain: A = sum_j rho^j M_(j+1) must be [tau] B, B = sum_j rho^j M_j, j < 4095
        uint8_t digest[32], ab[96];
        sha256_fast_prefixed(digest, (const uint8_t *)s->g1_values, n1 * sizeof(g1_t), (const uint8_t *)s->g2_values, n2 * sizeof(g2_t));
        const Fr rho = fr_from_digest(digest);
        std::vector<uint32_t> rows(2 * n1 * 8);
        power_row(rows.data(), rho, 1, n1 - 1);
        power_row(rows.data() + n1 * 8, rho, 0, n1 - 1);
        {
            std::lock_guard<std::mutex> lk(c->mu);
            LWK_HIP(hipSetDevice(c->device));
            C_KZG_RET rc = ctx_reserve(c, 2);
            if (rc != C_KZG_OK) return rc;
            hipStream_t st = c->stream;
            {
                WsUse wsu(c, st);
                LWK_HIP(hipMemcpyAsync(c->ws.scalars, rows.data(), 2 * n1 * 32, hipMemcpyHostToDevice, st));
                msm_stages(c, c->ws.scalars, c->ws.out48, 2, st);   // over the monomial form, on whatever engine it has
                LWK_HIP(hipMemcpyAsync(ab, c->ws.out48, 96, hipMemcpyDeviceToHost, st));
            }
            LWK_HIP(hipStreamSynchronize(st));
        }
        G1Affine pa, pb;
        pa.x = pa.y = pb.x = pb.y = Fp::zero();
        if (g1_decompress_nocheck(pa, ab) != 0 || g1_decompress_nocheck(pb, ab + 48) != 0) return C_KZG_OK;   // (a sum at infinity: no setup gives one)
        {
            const G1Affine ps[2] = {pa, {pb.x, neg(pb.y)}};
            const Fp2 x2[2] = {qx[0], qx[1]}, y2[2] = {qy[0], qy[1]};
            if (!pairing_product_is_one_uncached(ps, x2, y2, 2)) return C_KZG_OK;
        }
        // the G2 chain: g2[k + 1] = [tau] g2[k], with M_1 = [tau] M_0 (the generator) from the chain above
        for (size_t k = 0; k + 1 < n2; k++) {
            const G1Affine ps[2] = {m1, {m0.x, neg(m0.y)}};
            const Fp2 x2[2] = {qx[k], qx[k + 1]}, y2[2] = {qy[k], qy[k + 1]};
            if (!pairing_product_is_one_uncached(ps, x2, y2, 2)) return C_KZG_OK;
        }
        *ok = true;
        return C_KZG_OK;
    });
}

C_KZG_RET free_trusted_setup(KZGSettings *s) {
    if (!s) return C_KZG_OK;
    bool loaded = false;
    Ctx *c = registry_take(s, &loaded);   // (engine.hip: a loaded setup's own context, or the cached one of hand-built settings)
    ctx_destroy(c);
    free(s->g1_values);  // lib.rs:824-826
    free(s->g2_values);
    s->fs = nullptr;
    s->g1_values = nullptr;
    s->g2_values = nullptr;
    return C_KZG_OK;
}

// A KZGSettings filled in by hand (fs == NULL, caller-owned arrays: the reference's own layout) gets a device context
// on first use, cached by its g1_values pointer. free_trusted_setup would free() the caller's arrays; this drops only
// the cached context (tables, workspace, streams). The settings stay usable: the next call builds a new one.
C_KZG_RET lwkzg_release_context(const KZGSettings *s) {
    if (!s) return C_KZG_BADARGS;
    bool loaded = false;
    Ctx *c = registry_take(s, &loaded);
    if (loaded) return C_KZG_BADARGS;  // a loaded setup: free_trusted_setup owns it
    ctx_destroy(c);   // (nullptr: nothing was cached)
    return C_KZG_OK;
}

// ------------------------------------------------------------------------------------------------
// multi-GPU setup hand-off: [hdr 64][g1_values 589,824][g2_values 18,720 -> padded][table][tw_fwd][tw_inv][points]

static constexpr size_t kImgHdr = 64;
static constexpr size_t kImgG1 = (size_t)kBlobElems * 144;
static constexpr size_t kImgG2 = ((size_t)TRUSTED_SETUP_NUM_G2_POINTS * 288 + 63) / 64 * 64;
static constexpr size_t kImgTable = (size_t)kTablePoints * sizeof(G1Affine29);
static constexpr size_t kImgTw = (size_t)(kBlobElems / 2) * sizeof(Fr);
static constexpr size_t kImgPoints = (size_t)kBlobElems * sizeof(G1Affine);
static constexpr size_t kImgBytes = kImgHdr + kImgG1 + kImgG2 + kImgTable + 2 * kImgTw + kImgPoints;

size_t lwkzg_setup_image_bytes(void) { return kImgBytes; }

C_KZG_RET lwkzg_setup_export_device(const KZGSettings *s, void *image_dev, void *stream) {
    Ctx *c = ctx_of(s);
    if (!c || !image_dev) return C_KZG_ERROR;
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    uint8_t *img = (uint8_t *)image_dev;
    uint64_t hdr[8] = {kCtxMagic, kImgBytes, (uint64_t)kWindowBits, (uint64_t)kNumWindows, (uint64_t)P29::W, 0, 0, 0};
    LWK_HIP(hipMemcpyAsync(img, hdr, sizeof hdr, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemcpyAsync(img + kImgHdr, s->g1_values, kImgG1, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemsetAsync(img + kImgHdr + kImgG1, 0, kImgG2, st));
    LWK_HIP(hipMemcpyAsync(img + kImgHdr + kImgG1, s->g2_values, (size_t)TRUSTED_SETUP_NUM_G2_POINTS * 288, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemcpyAsync(img + kImgHdr + kImgG1 + kImgG2, c->table, kImgTable, hipMemcpyDeviceToDevice, st));
    LWK_HIP(hipMemcpyAsync(img + kImgHdr + kImgG1 + kImgG2 + kImgTable, c->tw_fwd, kImgTw, hipMemcpyDeviceToDevice, st));
    LWK_HIP(hipMemcpyAsync(img + kImgHdr + kImgG1 + kImgG2 + kImgTable + kImgTw, c->tw_inv, kImgTw, hipMemcpyDeviceToDevice, st));
    LWK_HIP(hipMemcpyAsync(img + kImgHdr + kImgG1 + kImgG2 + kImgTable + 2 * kImgTw, c->points, kImgPoints, hipMemcpyDeviceToDevice, st));
    LWK_HIP(hipStreamSynchronize(st));  // the host sources above must stay valid until the copies ran
    return C_KZG_OK;
}

C_KZG_RET lwkzg_setup_import_device(KZGSettings *out, const void *image_dev) {
    if (!out || !image_dev) return C_KZG_BADARGS;
    Ctx *c = nullptr;
    C_KZG_RET rc = ctx_new(&c);
    if (rc != C_KZG_OK) return rc;
    const uint8_t *img = (const uint8_t *)image_dev;
    uint64_t hdr[8];
    g1_t *g1v = (g1_t *)malloc(kImgG1);
    g2_t *g2v = (g2_t *)malloc((size_t)TRUSTED_SETUP_NUM_G2_POINTS * 288);
    bool ok = g1v && g2v && hipMemcpy(hdr, img, sizeof hdr, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && (hdr[0] != kCtxMagic || hdr[1] != kImgBytes || hdr[2] != (uint64_t)kWindowBits || hdr[3] != (uint64_t)kNumWindows ||
               hdr[4] != (uint64_t)P29::W)) {  // the table's limb width is part of the format
        set_error("setup image header mismatch (different build or not an image)");
        ok = false;
    }
    ok = ok && hipMemcpy(g1v, img + kImgHdr, kImgG1, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(g2v, img + kImgHdr + kImgG1, (size_t)TRUSTED_SETUP_NUM_G2_POINTS * 288, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(c->table, img + kImgHdr + kImgG1 + kImgG2, kImgTable, hipMemcpyDeviceToDevice) == hipSuccess &&
         hipMemcpy(c->points, img + kImgHdr + kImgG1 + kImgG2 + kImgTable + 2 * kImgTw, kImgPoints, hipMemcpyDeviceToDevice) == hipSuccess;
    if (ok) ok = ctx_finish_fft(c) == C_KZG_OK;
    if (!ok) {
        if (!get_error()[0]) set_error("setup image import failed");
        free(g1v);
        free(g2v);
        ctx_destroy(c);
        return C_KZG_ERROR;
    }
    out->fs = &c->fs;
    out->g1_values = g1v;
    out->g2_values = g2v;
    direct_from_env(out);
    return C_KZG_OK;
}

}  // extern "C"
