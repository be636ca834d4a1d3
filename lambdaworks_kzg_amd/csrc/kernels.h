// kernels.h -- host-side launchers of the HIP kernels (one per pipeline stage).
// Every launcher only enqueues work on `st`; nothing here synchronises or allocates.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include "g1.cuh"
#include "fr28.cuh"
#include "plan.h"
#include "mode_rules.h"
#include "recover_sets.h"

namespace lwk {

// ---- profiling hooks (engine.hip). Nothing is enqueued for them while profiling is off.
// ProfScope: a pair of marker packets (hipEventRecord) around whatever the scope enqueues on `st` -- several launches, or a copy.
// Where one such scope closes and the next opens on the same stream with NOTHING enqueued between them, one marker serves as both times:
// the first scope is built with kProfHandsOver, the second with kProfTakesOver -- the caller's word that it opens directly behind. The
// hand-over is per thread and lasts until the next scope or prof_launch of that thread, whichever it is.
constexpr unsigned kProfHandsOver = 1u, kProfTakesOver = 2u;
struct ProfScope {
    ProfScope(const char *name, hipStream_t st, unsigned link = 0);
    ~ProfScope();
    const char *name;
    hipStream_t st;
    hipEvent_t e0, e1;
    int dev;   // the device current at the scope's start: its events were created on it and go back to that device's pool
    unsigned link;
    bool on;
};
// prof_launch: ONE kernel launch under a profile name. Profiling on: the dispatch itself carries a pooled start and stop event
// (hipExtLaunchKernelGGL, flags 0: in stream order like any launch), so its time is the kernel's own and no marker packet sits between
// the launches of the region being timed. Profiling off, or LWKZG_PROF_MARKERS=1 (the A/B arm: ProfScope's marker pair on
// default-flag events): a plain hipLaunchKernelGGL.
bool prof_on();
bool prof_dispatch_events(hipEvent_t *e0, hipEvent_t *e1, int *dev);   // profiling is on; false: the marker arm, or no events to be had
void prof_dispatch_pending(const char *name, hipEvent_t e0, hipEvent_t e1, int dev);
template <typename... Formals, typename... Args>
inline void prof_launch(const char *name, hipStream_t st, void (*kernel)(Formals...), dim3 grid, dim3 block, uint32_t shmem, const Args &...args) {
    if (!prof_on()) {
        hipLaunchKernelGGL(kernel, grid, block, shmem, st, args...);
        return;
    }
    hipEvent_t e0, e1;
    int dev;
    if (prof_dispatch_events(&e0, &e1, &dev)) {
        hipExtLaunchKernelGGL(kernel, grid, block, shmem, st, e0, e1, 0, args...);
        prof_dispatch_pending(name, e0, e1, dev);
        return;
    }
    ProfScope p(name, st);
    hipLaunchKernelGGL(kernel, grid, block, shmem, st, args...);
}

// ---- scalar ingest (msm.hip)
// Mode R: 32-byte big-endian elements -> canonical 8xu32 little-endian limbs, reduced mod r
// (blob_to_polynomial, /root/reference/src/utils.rs:27-41).
// zero / zero2: up to two regions of words the launch clears on its way (fewer words each than there are elements)
void launch_parse_be_reduce(const uint8_t *blobs, uint32_t *scalars_raw, size_t n_elems, hipStream_t st, uint32_t *zero = nullptr, uint32_t zero_words = 0,
                            uint32_t *zero2 = nullptr, uint32_t zero2_words = 0);
// Mode C: 32-byte little-endian elements, must be canonical (else status[blob] = BADARGS) -> Montgomery Fr

// ---- MSM (msm.hip)
void launch_digit_sort(const uint32_t *scalars_raw, uint32_t *sorted, uint32_t *bucket_start, uint32_t *perm,
                       size_t n_blobs, hipStream_t st);
void launch_bucket_accumulate(const G1Affine29 *table, const uint32_t *sorted, const uint32_t *bucket_start,
                              const uint32_t *perm, G1Xyzz29 *buckets, size_t n_blobs, hipStream_t st);
void launch_bucket_reduce(const G1Xyzz29 *buckets, G1Xyzz29 *sums, size_t n_blobs, hipStream_t st);
// total (+)= sum of n points (tiled MSM partial results)
void launch_sum_points(const G1Xyzz29 *in, size_t n, G1Xyzz29 *total, int accumulate, hipStream_t st);
// sums -> 48-byte compressed points (compress_g1_point, /root/reference/src/compression.rs:33-60)
void launch_finalize_compress(const G1Xyzz29 *sums, uint8_t *out48, size_t n, hipStream_t st);

// ---- direct fixed-base MSM (direct.hip): every multiple d * 2^(bits j) * P_i precomputed, no buckets.
// bits in 10 .. 16; the table has direct_table_entries(bits) rows of 112 bytes, kDirectRowAligned or kDirectRowPacked apart
// (packed: 6 / 11 / 21 / 36 / 68 / 135 / 240 GB); 0 rows for any other width.
constexpr int kDirectMinBits = 10, kDirectMaxBits = 16;
// bytes from one row of the direct table to the next: 128 = every row in a 128-byte line of its own (a gather touches one
// line; +2.5 % at 13 bits, +5 % at 15, +1.4 % at 16, profiles/r02_experiments.md section 9), or 112 = the affine point
// itself, packed (7 of 8 rows straddle two lines), when the aligned table would not leave headroom in HBM
constexpr size_t kDirectRowAligned = 128, kDirectRowPacked = 112;
constexpr size_t kDirectAlignedHeadroom = (size_t)8 << 30;  // what an aligned table must leave free (two workspaces, verification scratch, the caller's buffers)
size_t direct_table_entries(int bits);
int direct_num_windows(int bits);
// The table is ONE ALLOCATION PER WINDOW: a hipMalloc that needs memory released shortly before (by the previous process, or by the table
// this one replaces) waits for the driver's scrub of it, ~25 ms per GB (profiles/r03_alloc_pieces.txt), so window j + 1 is being allocated
// by the host while the GPU builds window j, and the build costs max(wait, kernels) instead of their sum. The kernels index `win_dev`, the windows' base addresses in device memory.
constexpr int kDirectMaxWindows = 26;  // 10-bit windows
struct DirectTable {
    void *win[kDirectMaxWindows] = {};  // rows of window j: 4096 * 2^(bits-1) (the top window: 4096 * 2^wtop) rows of row_bytes
    uint64_t *win_dev = nullptr;        // the same addresses on the device
    int nw = 0;
    size_t bytes = 0;
};
// ms[0] = scratch allocations, ms[1] = the windows' hipMallocs (summed), ms[2] = what was left of the build kernels after the
// last allocation returned, ms[3] = freeing the scratch (host wall clock; may be null). On failure nothing stays allocated.
// in_place: keep the window allocations `table` already has (same width, same row size) and only run the build kernels over them
hipError_t build_direct_table(int bits, const G1Affine *points, DirectTable &table, size_t row_bytes, hipStream_t st, double *ms = nullptr,
                              bool in_place = false);
void free_direct_table(DirectTable &table);
// sums[b] = sum_i scalars[b][i] * P_i. `partials` needs up to 64 * n_blobs entries when a blob is spread over several workgroups (unused
// otherwise); `lane_scratch` 4096 * n_blobs entries (the per-lane sums of the hand-scheduled kernel) and `redo` n_blobs words (its flags).
// fill: workgroups to aim for (0 = 512, the right number when the kernel has the chip alone; see direct.hip).
void launch_direct_msm(int bits, const uint64_t *win_dev, size_t row_bytes, const uint32_t *scalars_raw, G1Xyzz29 *lane_scratch,
                       G1Xyzz29 *partials, uint32_t *redo, G1Xyzz29 *sums, size_t n_blobs, hipStream_t st, int fill = 0,
                       uint32_t *redo_flag_out = nullptr);
// the same, with the compressed sums in out48 as well where the launch set can leave them itself (one workgroup per blob on the
// hand-scheduled kernel: the fold, the inversion and the compression are one launch, k_commit_tail). Returns false where it could not:
// sums[] are complete as after launch_direct_msm, out48 is untouched and launch_finalize_compress is the caller's.
// redo_cleared: a kernel in front of this launch set on `st` has cleared redo[0 .. n_blobs) (launch_parse_be_reduce's second region)
bool launch_direct_msm_compressed(int bits, const uint64_t *win_dev, size_t row_bytes, const uint32_t *scalars_raw, G1Xyzz29 *lane_scratch,
                                  G1Xyzz29 *partials, uint32_t *redo, G1Xyzz29 *sums, uint8_t *out48, size_t n_blobs, hipStream_t st,
                                  int fill = 0, bool redo_cleared = false);
uint32_t direct_one_blob_counter_words(int bits);   // r06: see direct.hip
// sums[b] recomputed for the blobs with only_if[b] != 0 (one workgroup each, complete branches; exits at once for the others)
void launch_direct_msm_only(int bits, const uint64_t *win_dev, size_t row_bytes, const uint32_t *scalars_raw, G1Xyzz29 *sums,
                            const uint32_t *only_if, size_t n_blobs, hipStream_t st);

// ---- setup (setup.hip)
// 48-byte compressed -> affine Montgomery + status (0 ok, 1 infinity, 2 invalid); optional [r]P check
void launch_g1_decompress(const uint8_t *in48, G1Affine *out, int32_t *status, size_t n, int subgroup_check,
                          hipStream_t st);
// reference blst_p1 (canonical big-endian-limb x, y; z ignored) -> affine Montgomery, curve check
// (blst_p1_to_g1_point, /root/reference/src/srs.rs:155-172)
void launch_g1_from_blst(const uint64_t *blst_p1, G1Affine *out, int32_t *status, size_t n, hipStream_t st);
// affine Montgomery -> reference blst_p1 layout (g1_point_to_blst_p1, /root/reference/src/srs.rs:131-153)
void launch_g1_to_blst(const G1Affine *in, const int32_t *status, uint64_t *blst_p1, size_t n, hipStream_t st);
// T[j][i] = 2^(13 j) P_i
void launch_build_table(const G1Affine *points, G1Affine29 *table, hipStream_t st);

// ---- Fr (fr_ops.hip)
// twiddle table: w^-k (inverse) and w^k (forward), k < 2048, Montgomery; built once on device
void launch_build_twiddles(Fr *tw_fwd, Fr *tw_inv, hipStream_t st);
// in-place-in-LDS 4096-point radix-2 DIT over Fr. Input is consumed in the order given
// (bit-reversed-order input -> natural-order output). `scale_raw_out`: if set, output is multiplied by
// 4096^-1 and written as canonical raw limbs; otherwise Montgomery.
void launch_twiddles_to28(const Fr *tw, Fr28 *tw28, hipStream_t st);
void launch_ntt4096(const Fr *in, Fr *out, const Fr28 *tw28, int inverse_scale_to_raw, size_t n_blobs, hipStream_t st);
void launch_blob_evaluations_to_coefficients(const uint8_t *blobs, uint32_t *coeffs_raw, const Fr28 *tw28_inv, int32_t *status,
                                             size_t n_blobs, hipStream_t st, int le = 1);   // le = 0: canonical big-endian elements (eth mode)
void launch_bitrev_permute(const Fr *in, Fr *out, size_t n_blobs, hipStream_t st);
// c-kzg mode on the Lagrange form of the setup (fr_ops.hip): the 4096 rows of inverse-DFT coefficients whose
// commitments are the Lagrange points; the copy + range check that replaces the transform in front of a commitment; and the forward
// transform of a proof's quotient when only the Lagrange-form table exists
void launch_idft_columns(uint32_t *coeffs_raw, const Fr *tw_inv, uint32_t first, size_t n_rows, hipStream_t st);
// the opposite direction (a c-kzg setup arrives in Lagrange form): row b = the forward-DFT coefficients w^((first + b) bitrev12(k)), k < 4096,
// whose MSM over the Lagrange form is the monomial point [tau^(first + b)]G
void launch_dft_rows(uint32_t *coeffs_raw, const Fr *tw_fwd, uint32_t first, size_t n_rows, hipStream_t st);
void launch_copy_le_check(const uint8_t *blobs, uint32_t *scalars_raw, int32_t *status, size_t n_blobs, hipStream_t st);
// eth mode's twin: canonical big-endian elements -> the same least-significant-first limbs, the same range check
void launch_copy_be_check(const uint8_t *blobs, uint32_t *scalars_raw, int32_t *status, size_t n_blobs, hipStream_t st);
void launch_coefficients_to_evaluations(uint32_t *coeffs_raw, Fr *scratch, Fr *scratch2, const Fr28 *tw28_fwd, size_t n_blobs, hipStream_t st);
void launch_fr_be_to_mont(const uint8_t *in_be, Fr *out, size_t n_elems, hipStream_t st);
void launch_fr_mont_to_be(const Fr *in, uint8_t *out_be, size_t n_elems, hipStream_t st);
void launch_raw_to_be(const uint32_t *raw, uint8_t *out_be, size_t n_elems, hipStream_t st);
void launch_fr_mont_to_bytes(const Fr *in, uint8_t *out, int le, size_t n, hipStream_t st);
// y = p(z) and q = (p - y)/(x - z) per blob (Polynomial::evaluate + ruffini_division, call sites
// /root/reference/src/lib.rs:320,329,389,394). coeffs_raw/quot_raw: canonical limbs. y_out: 32 bytes,
// big-endian (le = 0) or little-endian (le = 1); may be NULL.
// only_if (optional): one word per blob; blobs whose word is zero are left as they are (a second pass over a few blobs)
// quot_raw = NULL: only y is computed (batch verification: a third of the products less)
void launch_eval_quotient(const uint32_t *coeffs_raw, const Fr *z_mont, uint32_t *quot_raw, uint8_t *y_out, int le,
                          size_t n_blobs, hipStream_t st, const uint32_t *only_if = nullptr);
// y = p(z) of reference-mode blobs straight from their bytes, any number in one launch (batch verification)
void launch_eval_y_from_blobs_be(const uint8_t *blobs, const Fr *z_mont, uint8_t *y_out, size_t n_blobs, hipStream_t st);
void launch_eval_y_from_blobs_evalform(const uint8_t *blobs, const Fr *z_mont, const Fr28 *roots_brp28, uint8_t *y_out, int32_t *status,
                                       size_t n_blobs, hipStream_t st, int le = 1);   // le = 1 (c-kzg mode): little-endian evaluations, range-checked; le = 0 (eth mode): big-endian, range-checked
// the same in evaluation form (c-kzg mode on the Lagrange form): evaluations in, the quotient's evaluations out, y = p(z) by the barycentric formula
// roots_brp28: the 4096 domain points in element order (launch_roots_brp28 writes them from the transform's twiddles, once per setup)
void launch_roots_brp28(const Fr28 *tw28_fwd, Fr28 *roots_brp28, hipStream_t st);
void launch_eval_quotient_evalform(const uint32_t *evals_raw, const Fr *z_mont, const Fr28 *roots_brp28, uint32_t *quot_raw, uint8_t *y_out, int le,
                                   size_t n_blobs, hipStream_t st, const uint32_t *only_if = nullptr);
// flags[i] = (a[48 i ..] != b[48 i ..])
void launch_flag_differs48(const uint8_t *a, const uint8_t *b, uint32_t *flags, size_t n, hipStream_t st);
// z bytes -> Montgomery. scalar_rule (mode_rules.h): kScalarBeReduced = big-endian, reduced; kScalarLeCanonical = little-endian, must be
// canonical else BADARGS; kScalarBeCanonical = big-endian, must be canonical else BADARGS. A digest is read with status = NULL and the
// byte order alone (ModeRules::le(), 0 or 1): reduced silently
void launch_z_from_bytes(const uint8_t *z_bytes, Fr *z_mont, int32_t *status, int scalar_rule, size_t n, hipStream_t st);

// ---- point validation (validate.hip)
// one set of compressed G1 points on its way through the validation: in48 -> pts / kind (0 = affine, 1 = infinity, 2 = invalid), the
// canonical bytes, and (optional) one word of scratch per point for the verdicts of the quad-of-lanes subgroup test
struct PointSet {
    const uint8_t *in48;
    G1Affine29 *pts;
    int32_t *kind;
    uint8_t *canon48;
    uint32_t *verdict;
};
// validate + canonicalise commitments (decompress incl. subgroup check, recompress: what compute_challenge hashes,
// /root/reference/src/utils.rs:120-154).
// verdict_scratch (n words, with aff_out and kind_out): the validation runs as three launches with the subgroup test on a quad of
// lanes per point (k_subgroup_coop_asm) instead of one lane per point for the whole chain
// apart (r06): the launches carry an LDS footprint they never touch, sized so that the dispatcher cannot place their workgroups on the
// compute units of a challenge-hash kernel running beside them (knobs.h: verify_pad_kb; profiles/r06_experiments.md section 1; lds_pad.h)
void launch_validate_commitments(const uint8_t *comm48, uint8_t *canon48, int32_t *status, int bad_code, size_t n,
                                 hipStream_t st, G1Affine29 *aff_out = nullptr, int32_t *kind_out = nullptr, uint32_t *verdict_scratch = nullptr,
                                 bool apart = false);
// the same in two steps, each ONE launch per kernel over one point set or two (b: a verification's proofs and commitments together): the
// linear combinations' multiples can start after the first. One set without verdict scratch, or validate_coop off: k_subgroup_canon alone
void launch_decompress_points(const PointSet &a, const PointSet *b, size_t n, hipStream_t st, bool apart = false);
// behind_decompress: the caller enqueues nothing on `st` between launch_decompress_points and this call (the two padded launches' profile
// scopes then share one marker)
void launch_subgroup_canon(const PointSet &a, const PointSet *b, int32_t *status, int bad_code, size_t n, hipStream_t st, bool apart = false,
                           bool behind_decompress = false);

// ---- the verification's linear combinations, r05's arm (setup.hip)
// verify side: three variable-base linear combinations in one launch (setup.hip).
//   set 0 = sum r_i P_i, set 1 = sum rz_i P_i (P = proofs), set 2 = sum r_i C_i (C = commitments);
// per-block partial sums to partial[set * nblk + block]
size_t lincomb3_blocks(size_t n);  // workgroups (= partial sums) per set
// *_mult: [2^32]P, [2^64]P, [2^96]P of every point (3 n entries, launch_point_multiples), so that each scalar is cut
// into 32-bit pieces on lanes of their own
void launch_point_multiples(const G1Affine29 *pts_a, const int32_t *kind_a, G1Affine29 *mult_a, size_t n, hipStream_t st,
                            const G1Affine29 *pts_b = nullptr, const int32_t *kind_b = nullptr, G1Affine29 *mult_b = nullptr);  // a second set: one launch
void launch_lincomb3(const G1Affine29 *proofs, const int32_t *proof_kind, const G1Affine29 *proof_mult, const G1Affine29 *comms,
                     const int32_t *comm_kind, const G1Affine29 *comm_mult, const uint8_t *sc_r_be, const uint8_t *sc_rz_be,
                     G1Xyzz29 *partial, size_t n, hipStream_t st);
// ---- the verification's linear combinations as one latency-shaped bucket MSM (vmsm.hip, r06) ----------------------------------
constexpr int kVmsmDigits = 16;                  // byte digits of a 128-bit half scalar
constexpr int kVmsmRows = 2 * kVmsmDigits;       // rows per point: [2^(8 j)]P and [2^(8 j)](-phi(P)), j = 0..15
constexpr int kVmsmSteps = kVmsmDigits - 1;      // rows per half beyond the point itself
constexpr int kVmsmMaxTerms = 64;                // terms per slice (one workgroup of k_vmsm_accumulate), at most
constexpr size_t kVmsmPinBytes = 33 * 32 + 3 * 96 + 3 * 4 + 52;  // the pinned host block of a verification: powers up, sums down
// the same block under an asynchronous verification (verify_async.hip): behind the sums and their flags a skip word on its way up (1: the
// batch was rejected, every launch behind r exits at once) and sum r^i y_i (32 bytes, k_verify_ysum) on its way down
constexpr size_t kVmsmPinSums = 33 * 32, kVmsmPinInfs = kVmsmPinSums + 3 * 96, kVmsmPinSkip = kVmsmPinInfs + 3 * 4, kVmsmPinYsum = kVmsmPinSkip + 4;
static_assert(kVmsmPinYsum + 32 <= kVmsmPinBytes, "the asynchronous verification's words fit the pinned block");
constexpr int kVmsmPwSkip = 33, kVmsmPwYsum = 34, kVmsmPwSlots = 35;   // Fr-sized slots of vm_pw on the device: the 33 powers, the skip word, sum r^i y_i
constexpr int kVmsmListCap = 24;                 // rows of one digit value a slice lists before its lane falls back to a scan
// rows of two point sets in one launch, beside the challenge hash: tab_*[row * n + i]; tmp: 15 x 2n XYZZ, pre: 15 x 2n field elements
void launch_vmsm_multiples2(const G1Affine29 *pts_a, const int32_t *kind_a, G1Affine29 *tab_a, const G1Affine29 *pts_b,
                            const int32_t *kind_b, G1Affine29 *tab_b, G1Xyzz29 *tmp, F29<2> *pre, size_t n, hipStream_t st, bool apart = false);
// pw: 33 Fr in Montgomery form, r^(2^k) for k = 0..31 and r^first; sc_a / sc_b: 8 words per term (lo | hi of a_i = r^(first+i), b_i = a_i z_i)
// skip (here and in the two launches below; nullptr for every synchronous caller): a device word that, when set, makes the launch exit at once
void launch_vmsm_scalars(const uint8_t *z_bytes, int le, const Fr *pw, uint32_t *sc_a, uint32_t *sc_b, size_t n, hipStream_t st,
                         const uint32_t *skip = nullptr);
uint32_t vmsm_terms_per_slice(size_t n);
size_t vmsm_slices(size_t n);
size_t vmsm_max_slices(size_t cap);
// partial: 3 x vmsm_slices(n) x 256 XYZZ; list_cap <= kVmsmListCap (smaller only to force the overflow path in tests)
// sc_c: the scalars of the third sum (over tab_c) when they are not sc_a (the cell batch's weights of its distinct commitments)
void launch_vmsm_accumulate(const uint32_t *sc_a, const uint32_t *sc_b, const G1Affine29 *tab_p, const int32_t *kind_p,
                            const G1Affine29 *tab_c, const int32_t *kind_c, G1Xyzz29 *partial, size_t n, hipStream_t st,
                            const uint32_t *sc_c = nullptr, const uint32_t *skip = nullptr);
// bsum: 3 x 256 XYZZ; out96 / inf: the three sums, affine big-endian x | y and an infinity flag each (what launch_xyzz29_to_affine_be leaves)
void launch_vmsm_reduce(const G1Xyzz29 *partial, G1Xyzz29 *bsum, uint8_t *out96, int32_t *inf, size_t n, hipStream_t st,
                        const uint32_t *skip = nullptr);
// verify_async.hip: out32 = sum_{i < n} r^(first + i) y_i, canonical big-endian; y32: the y bytes in the mode's byte order (canonical), pw: as
// launch_vmsm_scalars takes it. One workgroup; skip as above
void launch_verify_ysum(const uint8_t *y32, int le, const Fr *pw, uint8_t *out32, size_t n, hipStream_t st, const uint32_t *skip = nullptr);
// records[160 i] = C_i | z_i | y_i | pi_i from the device-resident pieces; *first_bad = lowest index with a status word set (pre-set to 0xffffffff)
void launch_verify_records(const uint8_t *canon_c, const uint8_t *z32, const uint8_t *y32, const uint8_t *canon_p, const int32_t *status,
                           uint8_t *records, uint32_t *first_bad, size_t n, hipStream_t st);
// verify_each.hip: z / y of n openings checked by scalar_rule (c-kzg: little-endian, < r; eth: big-endian, < r; reference: big-endian,
// reduced) and written canonical in the mode's byte order; a rejected item gets bad_code in status
void launch_each_openings(const uint8_t *z_in, const uint8_t *y_in, uint8_t *z_out, uint8_t *y_out, int32_t *status, int bad_code,
                          int scalar_rule, size_t n, hipStream_t st);
// verify_openings.hip: launch_each_openings and launch_verify_records in ONE launch for a batch of openings. z_in / y_in (16-byte aligned)
// are read by scalar_rule and written canonical to z_out / y_out (where k_vmsm_scalars and k_verify_ysum read them; in place is fine);
// records[160 i] = canon_c | z_out | y_out | canon_p; a rejected scalar puts bad_code into status[i]; *first_bad (pre-set to 0xffffffff)
// = the lowest index whose status word is set, by the validation before this launch or by this launch
void launch_opening_records(const uint8_t *z_in, const uint8_t *y_in, const uint8_t *canon_c, const uint8_t *canon_p, uint8_t *z_out,
                            uint8_t *y_out, int32_t *status, int bad_code, int scalar_rule, uint8_t *records, uint32_t *first_bad, size_t n,
                            hipStream_t st);
void launch_xyzz29_to_affine_be(const G1Xyzz29 *in, uint8_t *out96, int32_t *inf, size_t n, hipStream_t st);

// ---- Fiat-Shamir (sha256.hip, sha256_host.hip)
// z = sha256("FSBLOBVERIFY_V1_" | le64(4096) | le64(0) | blob | commitment) as Fr (compute_challenge, /root/reference/src/utils.rs:120-154)
// hash_rule (mode_rules.h: ModeRules::hash_rule()) -- kHashDigestLe: the digest is read little-endian; kHashFieldsBe (eth mode): the degree field is be128(4096). The
// midstate takes the degree field's rule alone (be_fields); the finish never meets that field.
void launch_challenge(const uint8_t *blobs, const uint8_t *canon48, Fr *z_mont, int hash_rule, size_t n, hipStream_t st,
                      const uint8_t *only_if_differs_from = nullptr);
void launch_challenge_midstate(const uint8_t *blobs, uint32_t *midstate, size_t n, hipStream_t st, bool be_fields = false);
void launch_challenge_finish(const uint8_t *blobs, const uint8_t *canon48, const uint32_t *midstate, Fr *z_mont, int hash_rule, size_t n,
                             hipStream_t st);
// sha256_host.hip: host SHA-256 -- portable | with the SHA extensions when present | the same of prefix | msg without the concatenation
void sha256_host(uint8_t out[32], const uint8_t *msg, size_t len);
void sha256_fast(uint8_t out[32], const uint8_t *msg, size_t len);
void sha256_fast_prefixed(uint8_t out[32], const uint8_t *prefix, size_t prefix_len, const uint8_t *msg, size_t len);
// sha256_host.hip: digests[i] = SHA-256("FSBLOBVERIFY_V1_" | le64(4096) | le64(0) | blobs[i] | comms[i]) on host threads
void challenge_digests_host(uint8_t *digests32, const uint8_t *blobs, const uint8_t *comms48, size_t n, bool be_fields = false);   // be_fields (eth mode): | be128(4096) | in place of the two le64
double host_hash_rate();   // bytes per second the host threads hashed in their recent long jobs (sha256_host.hip)
void challenge_midstates_host(uint32_t *mid, const uint8_t *blobs, size_t n, bool be_fields = false);   // 8 words per blob: the hash state k_challenge_finish continues from

// ---- EIP-7594 cells (cells.hip)
constexpr int kCellElems = 64;        // field elements per cell
constexpr int kCellsPerBlob = 128;    // cells (and cell proofs) per blob: 8192 extended evaluations
// the wanted columns of a call for c of the 128: k[i], i < c, strictly ascending. By value to the kernels, as the
// recovery's shared set travels: no device buffer, no lifetime, no synchronisation between calls that follow each other on a stream
struct CellColumns {
    uint8_t k[kCellsPerBlob];
};
// canonical coefficients of n_blobs blobs -> their 128 cells each (n_blobs x 256 KiB), 32-byte elements little-endian (le) or
// big-endian; scratch, scratch2: 2 n_blobs x 4096 Fr each. cols (with c, its count): only cells cols->k[0 .. c) of every blob leave,
// compact (n_blobs x c x 2 KiB), through the exit kernel that takes the list; the entry and the two transforms are the same
void launch_cells_extend(const uint32_t *coeffs_raw, const Fr *tw_fwd, const Fr28 *tw28_fwd, Fr *scratch, Fr *scratch2, uint8_t *cells,
                         int le, size_t n_blobs, hipStream_t st, const CellColumns *cols = nullptr, uint32_t c = kCellsPerBlob);
// canonical coefficients of n_cells / 128 blobs -> the monomial quotient q_k = p div (X^64 - c_k) of every cell, canonical limbs in
// scalar set (blob * 128 + k), zero-padded to 4096
void launch_cells_quotients(const uint32_t *coeffs_raw, const Fr *tw_fwd, uint32_t *quot_raw, size_t n_cells, hipStream_t st);
// the same for cells cols.k[0 .. c) of n_blobs blobs alone: q of cell cols.k[i] in scalar set (blob * c + i)
void launch_cells_quotients_columns(const uint32_t *coeffs_raw, const Fr *tw_fwd, uint32_t *quot_raw, const CellColumns &cols, uint32_t c,
                                    size_t n_blobs, hipStream_t st);

// ---- the FK20 cell proof engine (fk20.hip, pieces in fk20.cuh)
// rows first .. first + n_rows of the 8192 scalar rows whose commitments over the monomial setup are the transformed bases (row 128 i + m:
// Y^_i[m]); roots_raw: w128^e, e < 128, canonical limbs
void launch_fk20_base_rows(uint32_t *rows_raw, const uint32_t *roots_raw, uint32_t first, size_t n_rows, hipStream_t st);
// the window table of `bits` (fk20.cuh: fk20_plan, fk20_row) over the 8192 bases, none of them at infinity
void launch_fk20_table(const G1Affine *bases, G1Affine29 *table, int bits, hipStream_t st);
// canonical coefficients of n_blobs blobs -> the 64 coefficient transforms A^_i of each as canonical MSM scalars [blob][m][i] (256 KiB per blob)
void launch_fk20_coeffs(const uint32_t *coeffs_raw, const Fr *tw_fwd, uint32_t *scalars_out, size_t n_blobs, hipStream_t st);
// E[m] = sum_i A^_i[m] Y^_i[m] of every blob, at e_out[128 blob + rev7(m)]
void launch_fk20_msm(const G1Affine29 *table, int bits, const uint32_t *scalars, G1Xyzz29 *e_out, size_t n_blobs, hipStream_t st);
// pts[128 blob ..]: E in bit-reversed positions -> the blob's 128 proof points in proof order; roots: the recoded roots (fk20.cuh);
// h_out (optional): h_0 .. h_63 of every blob
void launch_fk20_transforms(G1Xyzz29 *pts, const uint8_t *roots, G1Xyzz29 *h_out, size_t n_blobs, hipStream_t st);
// the finalize of a call that wants c columns: point 128 blob + cols.k[i] of pts, compressed, at out48[48 (c blob + i)]
void launch_fk20_columns_compress(const G1Xyzz29 *pts, const CellColumns &cols, uint32_t c, uint8_t *out48, size_t n_blobs, hipStream_t st);

// ---- EIP-7594 recovery (recover.hip)
// the index set of a recovery call, passed to its kernels by value: RecoverSet (recover_sets.h)
static_assert(kRecoverCells == (size_t)kCellsPerBlob, "recover_sets.h counts the cells of a blob as the kernels do");
constexpr size_t kRecoverTabElems = 4 * kCellsPerBlob;   // the per-call table of k_recover_setup, Fr elements
void launch_recover_setup(const RecoverSet &set, const Fr *tw_fwd, Fr *tab, hipStream_t st);
// cells: n_blobs x num_cells x 2048 bytes, blob-major, 16-byte aligned, in the byte order `le` names -> the 4096 canonical coefficients
// of every blob at coeffs_raw. scratch: n_blobs x 8192 Fr. status[blob] = bad_code where an element is not below r or no polynomial of
// degree < 4096 goes through the blob's cells
void launch_recover_coefficients(const uint8_t *cells, const RecoverSet &set, size_t num_cells, const Fr *tw_fwd, const Fr *tw_inv, const Fr *tab,
                                 Fr *scratch, uint32_t *coeffs_raw, int32_t *status, int bad_code, int le, size_t n_blobs, hipStream_t st);

// The mixed form: every blob its own set. A call's distinct sets live on the device, written there by k_recover_mixed_setup alone:
// per set a table as k_recover_setup's, the list k[] (128 bytes, 0xff behind the last given cell) and the mask (4 words).
struct RecoverSetsDev {
    Fr *tab;          // n_sets x kRecoverTabElems
    uint8_t *k;       // n_sets x 128
    uint32_t *given;  // n_sets x 4
};
// the masks of up to kRecoverSetupGroup sets, by value to one setup launch
constexpr size_t kRecoverSetupGroup = 128;
struct RecoverMasks {
    uint32_t given[kRecoverSetupGroup][kCellsPerBlob / 32];
};
// what the interpolation and the solve know of up to kRecoverGroup blobs that follow each other, by value to one launch of each:
// set[j] = the set of the group's blob j, cell0[j] = the cells of the group in front of its own
constexpr size_t kRecoverGroup = 256;
struct RecoverGroup {
    uint32_t set[kRecoverGroup];
    uint32_t cell0[kRecoverGroup];
};
// sets first .. first + n_sets of dev from their masks (n_sets <= kRecoverSetupGroup)
void launch_recover_mixed_setup(const RecoverMasks &masks, size_t first, size_t n_sets, const Fr *tw_fwd, const RecoverSetsDev &dev, hipStream_t st);
// as launch_recover_coefficients for the n_blobs <= kRecoverGroup blobs of g, whose n_cells cells follow each other at `cells`
void launch_recover_mixed_coefficients(const uint8_t *cells, const RecoverGroup &g, size_t n_cells, const Fr *tw_fwd, const Fr *tw_inv,
                                       const RecoverSetsDev &dev, Fr *scratch, uint32_t *coeffs_raw, int32_t *status, int bad_code, int le,
                                       size_t n_blobs, hipStream_t st);

// ---- EIP-7594 cell proof batch verification (cells_verify.hip)
// digests32[32 i] = SHA-256(le64(rows[i]) | le64(idx[i]) | cell i | proof i); status[i] = bad_code where an element of cell i is not below r.
// cells and proofs48 are read in 16-byte pieces (16-byte aligned)
void launch_cellv_digests(const uint8_t *cells, const uint8_t *proofs48, const uint32_t *rows, const uint64_t *idx, uint8_t *digests32,
                          int32_t *status, int bad_code, int le, size_t n, hipStream_t st);
// pw: as launch_vmsm_scalars takes it. a_mont[i] = r^i (Montgomery); sc_a / sc_b: the split forms of r^i and r^i c_{idx[i]};
// sc_c[j], j < m: the split form of the sum of r^i over the items perm_row[row_off[j] .. row_off[j + 1])
// m_dev (nullptr for every synchronous caller): m where only the device knows it (cell_group.hip) -- the weights' launch then covers n
// rows and m is not read. skip (here and below; nullptr for every synchronous caller): as the vmsm launches' skip word
void launch_cellv_scalars(const Fr *pw, const uint64_t *idx, const Fr *tw_fwd, Fr *a_mont, uint32_t *sc_a, uint32_t *sc_b,
                          const uint32_t *perm_row, const uint32_t *row_off, uint32_t *sc_c, size_t n, size_t m, hipStream_t st,
                          const uint32_t *m_dev = nullptr, const uint32_t *skip = nullptr);
// the weights alone, one workgroup per row of `rows` rows (the grouped call's concatenated rows: cells_verify_groups.hip)
void launch_cellv_row_weights(const Fr *a_mont, const uint32_t *perm_row, const uint32_t *row_off, uint32_t *sc_c, size_t rows, hipStream_t st,
                              const uint32_t *m_dev = nullptr, const uint32_t *skip = nullptr);
// slot_raw: 4096 canonical scalars, the first 64 the coefficients of sum_i r^i I_i(X), the rest zero. perm_col / col_off (129 words): the
// items by column; colcoef: 128 x 64 Fr of scratch. Under skip slot_raw is 4096 zero scalars (the MSM behind it takes no skip word).
// The two launches (k_cellv_columns, k_cellv_coeffs) serve a call of groups too (cells_verify_groups.hip): groups first .. first +
// groups - 1 of the call, one word of flag each (the batch's skip word is the flag of its one group), col_off the lists 128 j + k of the
// whole call, colcoef and slot_raw one 128 x 64 scratch and one slot per group of THIS launch
void launch_cellv_interpolant(const uint8_t *cells, const Fr *a_mont, const uint32_t *perm_col, const uint32_t *col_off, const Fr *tw_inv,
                              Fr *colcoef, uint32_t *slot_raw, int le, hipStream_t st, const uint32_t *flag = nullptr, size_t first = 0,
                              size_t groups = 1);
// cells_verify_async.hip: fault (2 n words) -- [i] keeps the digests' word of item i and takes proof i's verdict, [n + j] is distinct
// commitment j's -- from the kinds the validation left
void launch_cellv_fault_words(int32_t *fault, const int32_t *kind_p, const int32_t *kind_c, int bad_code, size_t n, hipStream_t st);
// The first visit of the calls that say WHERE a fault is (the cell verifier's batch and grouped calls, the synchronous grouped call): the
// fills of fault's first n words and of status, the digests (their word into fault[i]), both point sets decompressed and checked -- set_p
// the n proofs, set_c the distinct commitments padded to n; status takes subgroup_canon's mixed words, which nobody reads --, the fault
// words. digests_done: an event recorded between the digests and the validation (the synchronous call's timing line), or nullptr.
// Returns the fills' and the record's error; nothing is read back
hipError_t launch_cellv_first_visit(const uint8_t *cells, const uint64_t *idx, const uint32_t *rows, const PointSet &set_p, const PointSet &set_c,
                                    uint8_t *digests32, int32_t *fault, int32_t *status, int bad_code, int le, size_t n, hipStream_t st,
                                    hipEvent_t digests_done = nullptr);

// ---- grouping the items of a cell proof batch on the device (cell_group.hip, pieces in cell_group.cuh)
// Scratch and outputs of one grouping, all device memory. Capacities for n items over a table of `slots` slots (cell_group.cuh:
// group_table_slots): table slots words, slot_of n, slot_row slots, row_cnt n, col_cnt 128, head kGroupHeadWords; rows n, first_item n,
// distinct 48 n, perm_row n, row_off n + 1, perm_col n, col_off 129.
constexpr int kGroupHeadM = 0, kGroupHeadBad = 1, kGroupHeadErr = 2, kGroupHeadWords = 4;
struct CellGroupBufs {
    uint32_t *table, *slot_of, *slot_row;
    uint32_t *row_cnt, *col_cnt;   // col_cnt is ONE piece with head: col_cnt 128 words | head (a single fill clears them)
    // [kGroupHeadM] = m; [kGroupHeadBad] = ~(the lowest i with idx[i] >= 128), 0 when there is none (so that the fill's zero means
    // "none" and the lanes take a maximum); [kGroupHeadErr] != 0: a probe ran out of slots or met a slot no lane had claimed
    uint32_t *head;
    uint32_t *rows, *first_item, *perm_row, *row_off, *perm_col, *col_off;
    uint8_t *distinct;   // the m distinct commitments in order of first occurrence, then infinity encodings up to n
};
// the scratch of a grouping of up to cap items out of a Carver (carve.h) -- any type with its take(); the outputs stay the caller's
template <class Carver_>
inline void cell_group_carve(CellGroupBufs &g, Carver_ &cv, size_t cap, size_t slots) {
    cv.take(g.table, slots * 4);
    cv.take(g.slot_of, cap * 4);
    cv.take(g.slot_row, slots * 4);
    cv.take(g.row_cnt, cap * 4);
    cv.take(g.col_cnt, (128 + kGroupHeadWords) * 4);
    g.head = (uint32_t *)((uintptr_t)g.col_cnt + 128 * 4);
    cv.take(g.first_item, cap * 4);
}
// n commitments (48 bytes each, 8-byte aligned) and n indices -> rows, m, distinct, first_item and the two lists as group_items
// (cells_verify_api.hip) makes them on the host; the order inside a group of perm_row / perm_col is not defined. seed / hash_mask: of the
// slot hash (cell_group.cuh). Six launches and three fills on st; nothing is read back
void launch_cell_group(const uint8_t *comms48, const uint64_t *idx, size_t n, size_t slots, uint64_t seed, uint32_t hash_mask,
                       const CellGroupBufs &g, hipStream_t st);

// ---- the same for a call of g groups (cell_group.hip): what plan_groups (cell_groups_plan.h) makes on the host.
// The key of an item is (its group, its 48 bytes); the groups are the contiguous item ranges item_off[j] .. item_off[j + 1] - 1.
// Capacities for n items in g groups: table slots words, slot_of n, slot_row slots, row_cnt n, pre n + 1, head kGroupHeadWords and
// behind it col_cnt 128 g (ONE piece, one fill); item_off g + 1 (in), item_group n, gbad g, rows n (GROUP-LOCAL), row_base g + 1,
// first_item n, distinct 48 n (the groups' distinct commitments one after the other, then infinity encodings), perm_row n / row_off
// n + 1 over the M = row_base[g] concatenated rows, perm_col n / col_off 128 g + 1 (list 128 j + k).
// head[kGroupHeadM] = M; head[kGroupHeadErr] as above; gbad[j] != 0: an index of group j is not below 128 -- the group has no rows
// and no columns, its items' rows are 0 and they are in neither list.
struct CellGroupSegBufs {
    uint32_t *table, *slot_of, *slot_row, *row_cnt, *pre;
    uint32_t *head, *col_cnt;
    uint32_t *item_off, *item_group, *gbad, *rows, *row_base, *first_item, *perm_row, *row_off, *perm_col, *col_off;
    uint8_t *distinct;
};
// what a segmented grouping needs beyond a CellGroupBufs of the same capacity, whose scratch and outputs it shares (a verifier runs
// one grouping or the other, never both at once)
template <class Carver_>
inline void cell_group_seg_carve(CellGroupSegBufs &s, const CellGroupBufs &g, Carver_ &cv, size_t cap, size_t gcap) {
    s.table = g.table, s.slot_of = g.slot_of, s.slot_row = g.slot_row, s.row_cnt = g.row_cnt, s.first_item = g.first_item;
    s.rows = g.rows, s.perm_row = g.perm_row, s.row_off = g.row_off, s.perm_col = g.perm_col, s.distinct = g.distinct;
    cv.take(s.pre, (cap + 1) * 4);
    cv.take(s.head, (kGroupHeadWords + 128 * gcap) * 4);
    s.col_cnt = (uint32_t *)((uintptr_t)s.head + kGroupHeadWords * 4);
    cv.take(s.item_off, (gcap + 1) * 4);
    cv.take(s.item_group, cap * 4);
    cv.take(s.gbad, gcap * 4);
    cv.take(s.row_base, (gcap + 1) * 4);
    cv.take(s.col_off, (128 * gcap + 1) * 4);
}
// s.item_off holds the call's g + 1 offsets (valid: group_offsets_valid). Seven launches and four fills on st; nothing is read back.
// Two of the seven are launch_cell_group's own kernels (k_group_scan with s.pre, k_group_offsets over 128 g column lists), under this
// call's names in the profile (k_seg_scan, k_seg_offsets); the insertion shares its probe with k_group_insert
void launch_cell_group_seg(const uint8_t *comms48, const uint64_t *idx, size_t n, size_t g, size_t slots, uint64_t seed, uint32_t hash_mask,
                           const CellGroupSegBufs &s, hipStream_t st);
// the slice table of the call (cell_groups_plan.h: plan_slice_count / plan_slice): slice_off[3 g + 1], slices[slice_off[3 g]]; a
// group with gflag[j] != 0 has no slices. One workgroup. slice_off[3 g] -- the live slice count -- never exceeds max_slices
struct GroupSlice;
void launch_cell_group_slice_table(const uint32_t *item_off, const uint32_t *row_base, const uint32_t *gflag, GroupSlice *slices,
                                   uint32_t *slice_off, size_t g, size_t max_slices, hipStream_t st);

// ---- the same for the commitments of whole blobs (cell_blobs_group.hip, the steps in cell_blobs_group.h): what
// plan_blobs (cell_blobs_plan.h) makes on the host. nb <= kBlobGroupCap blobs in g groups; item_off: the groups' g + 1 offsets in
// ITEMS (128 per blob) in device memory, or nullptr for a batch (g == 1, one group of all blobs). One launch of one workgroup for
// the grouping, one grid-stride launch for the lists; nothing is read back. Each returns its launch's error
struct BlobGroupOut;
hipError_t launch_cell_blobs_group(const uint8_t *comms48, const uint32_t *item_off, size_t nb, size_t g, uint64_t seed, uint32_t hash_mask,
                                   const BlobGroupOut &o, hipStream_t st);
// the lists of the 128 nb expanded items from o's tables: idx, rows (group-local), perm_row, perm_col, item_group (a grouped call's)
// per item; col_off 128 g + 1; row_off M + 1 and first_item M, in items; and, in o.distinct, the infinity encodings behind the M
// distinct commitments up to 128 nb entries
struct BlobItemsOut {
    uint64_t *idx;
    uint32_t *rows, *perm_row, *perm_col, *item_group, *col_off, *row_off, *first_item;
};
hipError_t launch_cell_blobs_items(const BlobGroupOut &o, const uint32_t *item_off, size_t nb, size_t g, const BlobItemsOut &x, hipStream_t st);

}  // namespace lwk
