// control.hip -- the process-wide controls behind the C ABI: semantics mode, device count and selection, the profiling report, the runtime's
// first use, the clock probe and the timing report.
#include "engine_internal.h"

#include <stdio.h>
#include <string.h>

#include <atomic>
#include <string>
#include <vector>

namespace lwk {

// Process-wide semantics switch. Every entry point reads it ONCE, at its start; lwkzg_set_mode must not race calls
// whose result should be in a particular mode (documented in the header).
static std::atomic<int> g_mode{-1};

static int mode_now() {
    int m = g_mode.load(std::memory_order_relaxed);
    if (m < 0) {
        m = mode_known(knobs().mode) ? knobs().mode : LWKZG_MODE_REFERENCE;   // LWKZG_MODE
        int expect = -1;
        if (!g_mode.compare_exchange_strong(expect, m)) m = expect;
    }
    return m;
}

int mode_of(const KZGSettings *s) {
    if (s) {
        const int m = ctx_mode_override(s);   // (engine.hip: under the registry's lock)
        if (m >= 0) return m;
    }
    return mode_now();
}
}  // namespace lwk

using namespace lwk;

extern "C" {

int lwkzg_set_mode(int mode) {
    int prev = mode_now();
    if (!mode_known(mode)) return -1;
    g_mode.store(mode);
    return prev;
}
int lwkzg_get_mode(void) { return mode_now(); }

// Per-settings semantics: a settings object that was given a mode of its own answers in it whatever the process-wide
// default says (-1 gives it back to the default); every entry point resolves its mode ONCE, when it is entered.
// An explicit mode for a settings object also brings its tables to that mode's form (tables.hip: settings_follow_mode): the first switch
// to c-kzg mode derives the Lagrange form (about 50 ms) and builds a Lagrange direct table beside the monomial one if it fits (the
// default engine: 0.2-0.3 s, 41 GB more); when the two do not fit side by side (15 / 16 bits) the ONE table is rebuilt in the new
// mode's form -- the cost of a lwkzg_enable_direct_table call of that width (0.9 s of kernels at 16 bits plus whatever hipMalloc
// waits for). Nothing happens when the tables already suit the mode. The process-wide default (lwkzg_set_mode) never moves a table.
int lwkzg_settings_set_mode(const KZGSettings *s, int mode) {
    if (!mode_known(mode) && mode != -1) return -1;
    Ctx *c = ctx_of(s);  // hand-built settings get their context here
    if (!c) return -1;
    const int prev = lwk::mode_of(s);
    c->mode_override.store(mode, std::memory_order_relaxed);
    const int now = lwk::mode_of(s);
    if (now != prev && gpu_available()) settings_follow_mode(c, now);
    return prev;
}
int lwkzg_settings_get_mode(const KZGSettings *s) { return lwk::mode_of(s); }

int lwkzg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int lwkzg_set_device(int ordinal) {
    int n = lwkzg_device_count();
    if (ordinal < 0 || ordinal >= n) {
        set_error("lwkzg_set_device(%d): %d device(s) visible", ordinal, n);
        return -1;
    }
    set_default_device(ordinal);
    return 0;
}
const char *lwkzg_version(void) { return "lambdaworks_kzg_amd 0.2 (gfx950; direct-table MSM, 10..16-bit windows; bucket fallback c=13, 20 windows)"; }
const char *lwkzg_last_error(void) { return get_error(); }
int lwkzg_msm_window_bits(void) { return kWindowBits; }
int lwkzg_msm_num_windows(void) { return kNumWindows; }

void lwkzg_profile_enable(int on) {
    if (!on) prof_drain();
    prof_set_on(on != 0);
}
void lwkzg_profile_reset(void) {
    prof_drain();
    prof_reset();
}
size_t lwkzg_profile_report(char *buf, size_t cap) {
    prof_drain();
    std::string s = "{";
    bool first = true;
    for (auto &kv : prof_totals()) {
        char line[256];
        snprintf(line, sizeof line, "%s\"%s\": {\"launches\": %llu, \"total_ms\": %.6f}", first ? "" : ", ",
                 kv.first.c_str(), (unsigned long long)kv.second.launches, kv.second.total_ms);
        s += line;
        first = false;
    }
    s += "}";
    if (buf && cap) {
        size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size() + 1;
}

size_t lwkzg_profile_sources(char *buf, size_t cap) {
    const ProfSources p = prof_sources();
    char s[256];
    const int n = snprintf(s, sizeof s, "{\"dispatch_pairs\": %llu, \"marker_pairs\": %llu, \"shared_markers\": %llu, \"event_flags\": %u}",
                           (unsigned long long)p.dispatch_pairs, (unsigned long long)p.marker_pairs, (unsigned long long)p.shared_markers, p.event_flags);
    if (buf && cap) {
        const size_t k = (size_t)n < cap - 1 ? (size_t)n : cap - 1;
        memcpy(buf, s, k);
        buf[k] = 0;
    }
    return (size_t)n + 1;
}

// first use of the HIP runtime by this process (device context, this library's code object): what a fresh process pays
// once, whichever call comes first. Returns 0, or -1 without a GPU.
__global__ void k_runtime_init(int *p) {
    if (p) *p = 1;
}

extern "C" int lwkzg_last_proof_schedule(void) { return last_proof_schedule(); }

extern "C" int lwkzg_runtime_init(void) {
    if (!gpu_available()) return -1;
    if (hipSetDevice(default_device()) != hipSuccess || hipFree(nullptr) != hipSuccess) return -1;
    // the code object is loaded by asking about one of its kernels -- NOT by launching one: a launch here would have to go to
    // the NULL stream, and a process that has used the NULL stream once keeps a hardware queue for it, after which the
    // engine's sub-batch streams no longer run side by side (measured: the bucket engine's two overlapped sub-batches fell
    // from 61.8k to 52.0k ops/s behind a single one-thread launch on stream 0)
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, (const void *)k_runtime_init) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return 0;
}

// What shader clock does this box hold under a dense multiply-add stream? One wave per SIMD runs ~0.4 ms of dependent v_mad_u64_u32
// and reads the shader clock (clock64) and the 100 MHz wall clock (wall_clock64) around it; MHz = the ratio, averaged over the waves.
// bench.py prints it next to a hash of the GPU's uuid so that a profiles/ summary can be matched to the box a line came from (boxes
// of this pool differ by several per cent). Launched on a stream of its own -- never the NULL stream (see lwkzg_runtime_init).
__global__ __launch_bounds__(256) void k_clock_probe(unsigned long long *out, uint32_t iters, uint32_t seed) {
    uint64_t acc = seed + threadIdx.x;
    const uint32_t a = (seed * 2654435761u) | 1u, b = seed ^ 0x9e3779b9u;
    const long long c0 = clock64(), w0 = wall_clock64();
    for (uint32_t i = 0; i < iters; i++) {
#pragma unroll
        for (int k = 0; k < 64; k++) acc = (uint64_t)(uint32_t)acc * a + (acc >> 32) + b;
    }
    const long long c1 = clock64(), w1 = wall_clock64();
    if ((threadIdx.x & 63) == 0) {
        const unsigned w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        out[3 * w] = (unsigned long long)(c1 - c0);
        out[3 * w + 1] = (unsigned long long)(w1 - w0);
        out[3 * w + 2] = acc;
    }
}

extern "C" C_KZG_RET lwkzg_clock_probe_mhz(double *mhz) {
    if (!mhz) return C_KZG_BADARGS;
    *mhz = 0;
    if (!gpu_available()) {
        set_error("no GPU: lambdaworks_kzg_amd has no CPU fallback");
        return C_KZG_ERROR;
    }
    LWK_HIP(hipSetDevice(default_device()));
    const unsigned wgs = 256, waves = wgs * 4;
    unsigned long long *d = nullptr;
    hipStream_t st = nullptr;
    LWK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (hipMalloc((void **)&d, waves * 3 * sizeof(unsigned long long)) != hipSuccess) {
        hipStreamDestroy(st);
        return C_KZG_MALLOC;
    }
    std::vector<unsigned long long> h(waves * 3);
    hipError_t e = hipSuccess;
    for (int rep = 0; rep < 3 && e == hipSuccess; rep++) {   // (the last of three back-to-back launches is the one read)
        hipLaunchKernelGGL(k_clock_probe, dim3(wgs), dim3(256), 0, st, d, 250u, 12345u + rep);
        e = hipStreamSynchronize(st);
    }
    if (e == hipSuccess) e = hipMemcpy(h.data(), d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    hipFree(d);
    hipStreamDestroy(st);
    if (e != hipSuccess) {
        set_error("lwkzg_clock_probe_mhz: %s", hipGetErrorString(e));
        return C_KZG_ERROR;
    }
    double clk = 0, wall = 0;
    for (unsigned w = 0; w < waves; w++) {
        clk += (double)h[3 * w];
        wall += (double)h[3 * w + 1];
    }
    if (wall > 0) *mhz = clk / wall * 100.0;   // wall_clock64 ticks at 100 MHz
    return C_KZG_OK;
}

// JSON: where the milliseconds of this settings object's load and of its last table build went
extern "C" size_t lwkzg_timing_report(const KZGSettings *s, char *buf, size_t cap) {
    Ctx *c = ctx_of(s);
    char tmp[1024];
    int k = 0;
    if (c) {
        std::lock_guard<std::mutex> lk(c->mu);
        const LoadTiming &l = c->load_timing;
        const BuildTiming &b = c->last_build;
        k = snprintf(tmp, sizeof tmp,
                     "{\"load\": {\"context_ms\": %.3f, \"points_and_tables_ms\": %.3f, \"g2_and_fft_ms\": %.3f, \"default_table_ms\": %.3f, "
                     "\"lagrange_section_ms\": %.3f, \"derive_monomial_ms\": %.3f, \"cross_check_ms\": %.3f, "
                     "\"total_ms\": %.3f}, \"last_table_build\": {\"bits\": %d, \"row_bytes\": %zu, \"table_bytes\": %zu, \"free_old_ms\": %.3f, "
                     "\"table_malloc_ms\": %.3f, \"scratch_malloc_ms\": %.3f, \"kernels_ms\": %.3f, \"scratch_free_ms\": %.3f, \"total_ms\": %.3f, \"in_place\": %d}}",
                     l.context_ms, l.points_and_tables_ms, l.g2_and_fft_ms, l.default_table_ms, l.lagrange_section_ms, l.derive_monomial_ms, l.cross_check_ms, l.total_ms, b.bits, b.row_bytes, b.table_bytes,
                     b.free_old_ms, b.table_malloc_ms, b.scratch_malloc_ms, b.kernels_ms, b.scratch_free_ms, b.total_ms, (int)b.in_place);
    } else {
        k = snprintf(tmp, sizeof tmp, "{}");
    }
    if (buf && cap) {
        size_t n = (size_t)k < cap - 1 ? (size_t)k : cap - 1;
        memcpy(buf, tmp, n);
        buf[n] = 0;
    }
    return (size_t)k + 1;
}

}  // extern "C"
