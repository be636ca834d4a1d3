// load.hip -- a trusted setup's way in and out: load from bytes or a file, free, release of a cached context, and the device image that
// hands a loaded setup to another GPU.
#include "engine_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

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
