// engine_internal.h -- what crosses between the engine's own translation units, and nothing else. Included only by engine.hip,
// proof_calls.hip, verify_front.hip, verify_async.hip, control.hip, load.hip, host_api.hip, tables.hip and device_api.hip; the rest of the library (verify.hip,
// verify_each.hip, cells*_api.hip, cells_verify_each.hip, recover_api.hip, multi.hip) sees the engine through engine.h, the entry points'
// guard through abi_guard.h, the carver through carve.h and the EIP-7594 compute paths' shared code through cells_common.h.
#pragma once
#include "engine.h"
#include "knobs.h"

#include <map>
#include <string>

namespace lwk {

// ---- engine.hip: profiling (the state stays there) -------------------------------------------------------------------------------
struct ProfAgg {
    uint64_t launches = 0;
    double total_ms = 0;
};
void prof_drain();
void prof_set_on(bool on);
void prof_reset();                                // the event pools and the totals
std::map<std::string, ProfAgg> prof_totals();     // a copy, taken under the profiling lock
struct ProfSources {                              // since the last prof_reset
    uint64_t dispatch_pairs, marker_pairs, shared_markers;
    unsigned event_flags;                         // creation flags of the pooled event made last
};
ProfSources prof_sources();

// ---- engine.hip: registry, devices, context lifetime ------------------------------------------------------------------------------
int ctx_mode_override(const KZGSettings *s);                 // under the registry's lock; -1: none
Ctx *registry_take(const KZGSettings *s, bool *loaded);      // under the registry's lock
bool gpu_available();
int default_device();
void set_default_device(int ordinal);
C_KZG_RET ctx_new(Ctx **out, const Ctx *twin_of = nullptr);
void ctx_destroy(Ctx *c);
C_KZG_RET ctx_finish_fft(Ctx *c);
bool twin_off();
Ctx *pick_ctx(Ctx *c, hipStream_t st);
bool peer_busy(const Ctx *c);
void direct_from_env(const KZGSettings *s);

template <class T>
static void dev_free(T *&p) {
    if (p) hipFree(p);
    p = nullptr;
}

// A lane of the coalescing front uses ONE half of the workspace on its own stream: it waits for the last user of the
// whole workspace and leaves an event of its own; the two lanes do not wait for each other.
struct WsLaneUse {
    Ctx *c;
    int lane;
    WsLaneUse(Ctx *c_, int lane_) : c(c_), lane(lane_) { hipStreamWaitEvent(c->aux[lane], c->ws_done, 0); }
    ~WsLaneUse() {
        hipEventRecord(c->lane_done[lane], c->aux[lane]);
        c->ws_last = nullptr;  // the next whole-workspace user must wait for its predecessor's event again: a lane ran between
    }
};

// ---- engine.hip: the launch stages (msm_stages and coefficients_to_msm_form are in engine.h) --------------------------------------
G1Xyzz29 *msm_sums_stage(Ctx *c, const uint32_t *scalars_raw, size_t n, hipStream_t st, size_t base = 0, bool shared_chip = false,
                         bool lagrange = false, G1Xyzz29 *sums_out = nullptr, uint32_t *redo_flag_out = nullptr);
size_t host_finish_limit();
void host_finish_compress(uint8_t out[48], const G1Xyzz29 &sum);
bool proof_in_evaluation_form(const Ctx *c, int mode);
bool proof_on_lagrange(const Ctx *c, int mode);
void quotient_stage(Ctx *c, int mode, const uint32_t *in, const Fr *z, uint32_t *quot, uint8_t *y_out, int le, size_t n, hipStream_t st,
                    const uint32_t *only_if = nullptr);
bool quotient_to_msm_form(Ctx *c, int mode, size_t n, hipStream_t st, size_t base = 0);
bool coefficients_stage(Ctx *c, const uint8_t *blobs, size_t n, int mode, int32_t *status, hipStream_t st, size_t base = 0,
                        bool evaluations_ok = false, uint32_t *zero = nullptr, uint32_t zero_words = 0, uint32_t *zero2 = nullptr,
                        uint32_t zero2_words = 0);

C_KZG_RET first_status(Ctx *c, const int32_t *d_status, size_t n, hipStream_t st);

// ---- proof_calls.hip: the device-resident proof pipelines not in engine.h, their pinned staging and their per-call scratch --------
C_KZG_RET commit_and_prove_batch_device(Ctx *c, uint8_t *comm_out48, uint8_t *proof_out48, const uint8_t *blobs, size_t n, int mode,
                                        hipStream_t st, int32_t *status);
int last_proof_schedule();
size_t small_proof_host_limit();
size_t mid_proof_host_limit();
bool sph_reserve(Ctx *c, size_t n, bool at_reserve = false);
void sph_free(SmallProofHost &h);
// Where the per-blob words of a call of n blobs live: the workspace's own arrays up to one chunk (ctx_reserve has run), the context's
// long block -- reserved here, grow-only, a separate allocation -- beyond. `status` is the caller's array when it passes one. Caller holds c->mu.
struct CallWords {
    int32_t *status;
    Fr *z;
    uint8_t *canon;
    G1Affine29 *val_pts;   // the validation's scratch: this, val_kind and val_verdict
    int32_t *val_kind;
    uint32_t *val_verdict;
};
C_KZG_RET call_words(Ctx *c, size_t n, int32_t *caller_status, CallWords &out);

// ---- engine.hip: context-owned grow-only buffers that several files share (caller holds c->mu) -----------------------------------
uint8_t *host_res_block(Ctx *c, size_t bytes);
hipStream_t upload_stream(Ctx *c);
bool dev_stage_ready(Ctx *c);
size_t stage_slice_len(size_t k, size_t remaining);
C_KZG_RET stage_upload(Ctx *c, size_t k, const uint8_t *src, size_t cnt, hipStream_t compute, uint8_t **d_blobs);
C_KZG_RET stage_parsed(Ctx *c, size_t k, hipStream_t compute);

// ---- verify_front.hip -------------------------------------------------------------------------------------------------------------
void vs_free(Ctx *c);

// ---- tables.hip -------------------------------------------------------------------------------------------------------------------
void settings_follow_mode(Ctx *c, int mode);
C_KZG_RET enable_direct_table(const KZGSettings *s, int window_bits, size_t row_pref, int forms = 0);
// A setup that arrives in Lagrange form (load.hip: the c-kzg loaders; the context is not published yet, no lock is needed).
// lagrange_from_bytes: 4096 compressed points ALREADY in the blob's bit-reversed order on the device -> lag.points (decompressed, subgroup
// check, verdicts in d_status) and lag.table, enqueued on the context's stream. monomial_from_lagrange: the 4096 compressed monomial
// points at d_comp48, kMaxChunk rows of forward-DFT coefficients at a time over that table (twiddles and workspace must exist).
// lagrange_publish: the form is live (lagrange_prepare finds nothing to do).
C_KZG_RET lagrange_from_bytes(Ctx *c, const uint8_t *d_in48, int32_t *d_status);
C_KZG_RET monomial_from_lagrange(Ctx *c, uint8_t *d_comp48);
void lagrange_publish(Ctx *c);
// the Lagrange form of a published settings object, derived now if absent: lagrange_prepare under the locks settings_follow_mode takes
C_KZG_RET lagrange_ensure(Ctx *c);

}  // namespace lwk
