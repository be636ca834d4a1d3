/*
 * lambdaworks_kzg_amd.h -- C ABI of the MI355X-native KZG / EIP-4844 blob-commitment engine.
 *
 * Drop-in boundary for lambdaclass/lambdaworks_kzg's hot path. The first nine functions are
 * exactly the reference's `#[no_mangle] extern "C"` symbols (the c-kzg-4844 surface); a
 * maintainer links this library instead of liblambdaworks_kzg and keeps calling them.
 * Header of record on the reference side: src/c_kzg_4844.h:85-231 (NOT the stale
 * src/lambdaworks_kzg.h). Each declaration cites the Rust definition it replaces.
 *
 * Everything after "extensions" is additive: batched and device-resident entry points (a
 * synchronous one-blob call cannot reach 10k ops/s), the R/C semantics switch, multi-GPU setup
 * hand-off, EIP-7594 cells, cell proofs and their batch and per-item verification, and profiling hooks used
 * by bench.py.
 *
 * Struct layouts follow the reference's #[repr(C)] types (src/lib.rs:45-232). NOTE the
 * reference's blst_fp convention, which this library reproduces bit for bit and which is NOT
 * blst's: limbs hold the canonical (non-Montgomery) integer, most-significant limb first
 * (src/srs.rs:131-172; the reference's own test compares these structs, tests/lib_test.rs:153-163).
 */
#ifndef LAMBDAWORKS_KZG_AMD_H
#define LAMBDAWORKS_KZG_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden; these are its only exported symbols */
#pragma GCC visibility push(default)

#ifndef FIELD_ELEMENTS_PER_BLOB
#define FIELD_ELEMENTS_PER_BLOB 4096 /* fixed in the reference: src/lib.rs:76 */
#endif
#if FIELD_ELEMENTS_PER_BLOB != 4096
#error this engine is built for FIELD_ELEMENTS_PER_BLOB = 4096 (reference src/lib.rs:76)
#endif

#define BYTES_PER_COMMITMENT 48    /* src/lib.rs:67 */
#define BYTES_PER_PROOF 48         /* src/lib.rs:70 */
#define BYTES_PER_FIELD_ELEMENT 32 /* src/lib.rs:73 */
#define BYTES_PER_BLOB (FIELD_ELEMENTS_PER_BLOB * BYTES_PER_FIELD_ELEMENT) /* src/lib.rs:81 */
#define TRUSTED_SETUP_NUM_G1_POINTS FIELD_ELEMENTS_PER_BLOB                /* src/lib.rs:78 */
#define TRUSTED_SETUP_NUM_G2_POINTS 65                                     /* src/lib.rs:92 */

/* ---- blst-shaped types (src/lib.rs:100-166). Guarded so a real blst.h may come first. ---- */
#ifndef LWKZG_HAVE_BLST_TYPES
#ifndef __BLST_H__
typedef uint64_t limb_t;
typedef struct { limb_t l[256 / 8 / sizeof(limb_t)]; } blst_fr;
typedef struct { limb_t l[384 / 8 / sizeof(limb_t)]; } blst_fp;
typedef struct { blst_fp fp[2]; } blst_fp2;
typedef struct { blst_fp x, y, z; } blst_p1;
typedef struct { blst_fp x, y; } blst_p1_affine;
typedef struct { blst_fp2 x, y, z; } blst_p2;
typedef struct { blst_fp2 x, y; } blst_p2_affine;
#endif
#endif

typedef blst_p1 g1_t;
typedef blst_p2 g2_t;
typedef blst_fr fr_t;

typedef struct { uint8_t bytes[32]; } Bytes32;             /* src/lib.rs:94 */
typedef struct { uint8_t bytes[48]; } Bytes48;             /* src/lib.rs:95 */
typedef struct { uint8_t bytes[BYTES_PER_BLOB]; } Blob;    /* src/lib.rs:98 */
typedef Bytes48 KZGCommitment;                             /* src/lib.rs:96 */
typedef Bytes48 KZGProof;                                  /* src/lib.rs:97 */

typedef enum {
    C_KZG_OK = 0,  /* success */
    C_KZG_BADARGS, /* the supplied data is invalid in some way */
    C_KZG_ERROR,   /* internal error; the reference maps EVERY failure to this (src/lib.rs:263,267,272,...) */
    C_KZG_MALLOC,  /* could not allocate memory */
} C_KZG_RET;       /* src/lib.rs:45-57 */

typedef struct {
    uint64_t max_width;
    fr_t *expanded_roots_of_unity; /* w^i, i = 0..max_width (max_width + 1 entries) */
    fr_t *reverse_roots_of_unity;  /* w^-i, max_width + 1 entries */
    fr_t *roots_of_unity;          /* w^bitrev(i), max_width entries */
} FFTSettings;                     /* src/lib.rs:173-197 */

typedef struct {
    FFTSettings *fs;  /* reference: always NULL (src/lib.rs:754-758). Here: the engine's context; its
                         first member is a genuine FFTSettings (max_width = 4096). */
    g1_t *g1_values;  /* 4096 monomial points [tau^i]G, reference blst_fp convention, malloc'd */
    g2_t *g2_values;  /* 65 points [tau^i]G2, malloc'd */
} KZGSettings;        /* src/lib.rs:206-222 */

/* ============================ the reference's nine symbols ============================ */

/* src/lib.rs:709-776. n1 != 4096 or n2 != 65 -> C_KZG_BADARGS (the reference's only BADARGS). */
C_KZG_RET load_trusted_setup(KZGSettings *out, const uint8_t *g1_bytes /* n1*48 */, size_t n1,
                             const uint8_t *g2_bytes /* n2*96 */, size_t n2);

/* src/lib.rs:779-802 + src/srs.rs:25-128: line-based text format, decimal n1, n2, then hex points. */
C_KZG_RET load_trusted_setup_file(KZGSettings *out, FILE *in);

/* src/lib.rs:821-829. (c_kzg_4844.h:186 declares void; the Rust symbol returns C_KZG_OK.) */
C_KZG_RET free_trusted_setup(KZGSettings *s);

/* src/lib.rs:253-283 */
C_KZG_RET blob_to_kzg_commitment(KZGCommitment *out, const Blob *blob, const KZGSettings *s);

/* src/lib.rs:300-344 */
C_KZG_RET compute_kzg_proof(KZGProof *proof_out, Bytes32 *y_out, const Blob *blob, const Bytes32 *z_bytes,
                            const KZGSettings *s);

/* src/lib.rs:361-404 */
C_KZG_RET compute_blob_kzg_proof(KZGProof *out, const Blob *blob, const Bytes48 *commitment_bytes,
                                 const KZGSettings *s);

/* src/lib.rs:407-453 */
C_KZG_RET verify_kzg_proof(bool *ok, const Bytes48 *commitment_bytes, const Bytes32 *z_bytes, const Bytes32 *y_bytes,
                           const Bytes48 *proof_bytes, const KZGSettings *s);

/* src/lib.rs:456-505 */
C_KZG_RET verify_blob_kzg_proof(bool *ok, const Blob *blob, const Bytes48 *commitment_bytes,
                                const Bytes48 *proof_bytes, const KZGSettings *s);

/* src/lib.rs:525-614. n == 0 -> C_KZG_OK with *ok = false in reference mode (src/lib.rs:538-543) and *ok = true in
 * c-kzg mode (the reference's own vector verify_blob_kzg_proof_batch_case_a271b78b8e869d69) and in eth mode (the consensus specs).
 * Batches of more than 1024 blobs are uploaded into a device buffer of n * 131072 bytes that the settings object keeps (grow-only, freed by
 * free_trusted_setup): 4096 blobs 12.1 ms, of which 9.6 are the upload; lwkzg_verify_blob_kzg_proof_batch_device takes blobs that are
 * already in HBM (5.3 ms). */
C_KZG_RET verify_blob_kzg_proof_batch(bool *ok, const Blob *blobs, const Bytes48 *commitments_bytes,
                                      const Bytes48 *proofs_bytes, size_t n, const KZGSettings *s);

/* ==================================== extensions ==================================== */

/* Semantics switch.
 *   LWKZG_MODE_REFERENCE (default): what lambdaworks_kzg computes -- big-endian scalars are monomial
 *       coefficients (src/utils.rs:27-41), big-endian z/y and Fiat-Shamir digest, every failure is
 *       C_KZG_ERROR, scalars >= r are reduced.
 *   LWKZG_MODE_CKZG: what the c-kzg-4844 vectors under the reference's tests/ encode -- canonical
 *       little-endian scalars are evaluations on the bit-reversed 4096th roots of unity (inverse NTT
 *       in front of the same MSM), little-endian z/y/digest, invalid input is C_KZG_BADARGS.
 *   LWKZG_MODE_ETH ("consensus-specs mode"): the encoding of the consensus specs since Deneb, of c-kzg-4844 from 1.0 on and of every
 *       mainnet client -- c-kzg mode with BIG-endian canonical field elements (blob elements, z, y, cells, challenge outputs; an
 *       element, z or y not below r is C_KZG_BADARGS), the blobs evaluations on the bit-reversed domain, and the specs' transcripts:
 *       compute_challenge hashes "FSBLOBVERIFY_V1_" | be128(4096) | blob | commitment (8 zero bytes, then be64(4096)) and the batch
 *       challenge "RCKZGBATCH___V1_" | be64(4096) | be64(n) | n x (C | z | y | proof) with z and y big-endian; both digests are read
 *       big-endian and reduced. Every other rule is c-kzg mode's (infinity allowed as a commitment or proof, its non-canonical
 *       encodings re-hashed over the canonical bytes, C_KZG_BADARGS, an empty blob batch verifies, the z-on-the-domain branch). In
 *       this mode the bytes of commitments, proofs, y, cells, cell proofs and recovered cells, and the verdicts, are c-kzg-4844 2.x's.
 *       The mode runs on the Lagrange form of the setup exactly as c-kzg mode does: moving a settings object between the two moves
 *       or derives no table. (The cell batch's transcript stays the library's own in every mode -- see
 *       lwkzg_verify_cell_kzg_proof_batch: the per-cell digests use le64(row) | le64(k) and the header le64 fields; in eth mode only
 *       the reading of that digest into r, and the r bytes of the partials, follow the mode: big-endian. The spec's single
 *       sequential hash over n x 2112 bytes would put milliseconds of serial SHA-256 in front of the sums, and the verdict does not
 *       depend on it.)
 *   "The mode's byte order" in the notes below: big-endian in reference and eth mode, little-endian in c-kzg mode.
 * lwkzg_set_mode sets the process-wide DEFAULT (initial value from the environment variable LWKZG_MODE,
 * "reference"|"ckzg"|"eth"); lwkzg_settings_set_mode gives ONE settings object a mode of its own, which wins over the default
 * (mode -1 hands it back to the default), so two consumers in one process can use different semantics. Every entry
 * point resolves its mode once, when it is entered: a change does not affect calls already in flight.
 * Cost of lwkzg_settings_set_mode: it brings the settings' MSM tables to the new mode's form (lwkzg_direct_table_forms below). The
 * first switch to c-kzg mode derives the Lagrange form of the setup on the device (about 50 ms) and builds a second direct table
 * beside the first if it fits (default engine: 0.2-0.3 s and 41 GB more); at 15 / 16 bits, where only one table fits, the table is
 * REBUILT in the new form (what lwkzg_enable_direct_table of that width costs: 0.9 s of kernels at 16 bits plus the driver's
 * hipMalloc waits). Switching back and forth between two forms that both exist is free. lwkzg_set_mode never touches a table: a
 * settings object that merely follows the default gets the Lagrange form on its first c-kzg call, and only if it fits beside. */
#define LWKZG_MODE_REFERENCE 0
#define LWKZG_MODE_CKZG 1
#define LWKZG_MODE_ETH 2
int lwkzg_set_mode(int mode); /* returns the previous default, or -1 if `mode` is invalid */
int lwkzg_get_mode(void);
int lwkzg_settings_set_mode(const KZGSettings *s, int mode); /* returns the mode calls on `s` answered in before, -1 on error */
int lwkzg_settings_get_mode(const KZGSettings *s);           /* the mode a call on `s` would answer in now */

/* For a KZGSettings filled in by hand (fs == NULL and caller-owned g1_values / g2_values, the reference's own layout,
 * src/lib.rs:754-758): the library builds a device context for it on first use and caches it by the g1_values pointer
 * (re-checked against a digest of the first and last point). free_trusted_setup() would free() the caller's arrays; this
 * releases only the cached device context. C_KZG_BADARGS for a setup the library loaded itself. */
C_KZG_RET lwkzg_release_context(const KZGSettings *s);

/* Batched host-pointer forms of src/lib.rs:253 / :361 / :300: n blobs in, n results out, one launch
 * set. On failure nothing useful is in `out`; `first_bad` (may be NULL) receives the index of the
 * first offending blob. */
C_KZG_RET lwkzg_blob_to_kzg_commitment_batch(KZGCommitment *out, const Blob *blobs, size_t n, const KZGSettings *s,
                                             size_t *first_bad);
C_KZG_RET lwkzg_compute_blob_kzg_proof_batch(KZGProof *out, const Blob *blobs, const Bytes48 *commitments, size_t n,
                                             const KZGSettings *s, size_t *first_bad);
C_KZG_RET lwkzg_compute_kzg_proof_batch(KZGProof *proofs_out, Bytes32 *ys_out, const Blob *blobs, const Bytes32 *zs,
                                        size_t n, const KZGSettings *s, size_t *first_bad);

/* Device-resident forms: every pointer is a DEVICE pointer on the settings' GPU; `stream` is a
 * hipStream_t (NULL = the engine's own stream). Asynchronous: kernels are enqueued and the call
 * returns; per-blob status words (0 = ok, C_KZG_RET otherwise) are written to status_dev (n x int32,
 * may be NULL). No allocation happens here once lwkzg_reserve() has been called for >= n (proof calls of more than
 * 1024 blobs allocate n x 84 bytes once; the first blob-proof call of up to LWKZG_SMALL_PROOF_HOST = 128 blobs allocates its
 * pinned staging, 128 KiB per blob, and synchronises the device once -- such a call takes its Fiat-Shamir challenges and its
 * commitment validation from the host threads, in stream order through a host function, because the GPU's two latency
 * chains cost 3.6 ms however few the blobs are; the call still returns without waiting. Calls of up to LWKZG_MID_PROOF_HOST = 384
 * blobs on a settings object whose other caller stream is idle hash on the host too, in chunks beside the copy out, while the GPU
 * validates: 4.9 instead of 6.1 ms at 256 blobs). Calls on one settings object share its workspace: whatever `stream` each is
 * given, the library orders their GPU work one after the other (event dependencies, no host blocking), so two calls
 * in flight on two streams are safe and serial. A proof call hashes and validates ALL its blobs up front (two latency
 * chains of ~3 ms whose duration does not depend on n), then runs the MSMs chunk by chunk: one call of 4096 blobs
 * pays them once, four calls of 1024 four times. */
C_KZG_RET lwkzg_blob_to_kzg_commitment_batch_device(void *out48_dev, const void *blobs_dev, size_t n,
                                                    const KZGSettings *s, void *stream, int32_t *status_dev);
C_KZG_RET lwkzg_compute_blob_kzg_proof_batch_device(void *out48_dev, const void *blobs_dev, const void *commitments48_dev,
                                                    size_t n, const KZGSettings *s, void *stream, int32_t *status_dev);
/* Commitment AND blob proof of n device-resident blobs in one pass: commitments48_dev[i] = blob_to_kzg_commitment(blob_i),
 * proofs48_dev[i] = compute_blob_kzg_proof(blob_i, commitments48_dev[i]) -- src/lib.rs:253-283 followed by src/lib.rs:361-404
 * on its own output, byte for byte what the two calls above return. What a blob producer needs, ~15 % faster than the two
 * calls: the part of the Fiat-Shamir hash that does not depend on the commitment runs beside the commitment MSM, and the
 * blob is parsed once. status_dev as above. */
C_KZG_RET lwkzg_commit_and_prove_batch_device(void *commitments48_dev, void *proofs48_dev, const void *blobs_dev, size_t n,
                                              const KZGSettings *s, void *stream, int32_t *status_dev);
C_KZG_RET lwkzg_reserve(const KZGSettings *s, size_t max_batch);
/* lwkzg_reserve covers calls on ONE caller stream. A device-resident call that arrives on a second stream while the
 * workspace is busy runs on a second context of the settings object (own streams and workspace, about 1.8 MB per blob of
 * max_batch, over the same tables); unless reserved here it is created inside that first overlapped call, which then
 * allocates and synchronises the device once. caller_streams >= 2 creates and reserves it now. Footprint of a load beside
 * this: the default engine's table (41 GB when the device is empty, see lwkzg_enable_direct_table below). */
C_KZG_RET lwkzg_reserve_streams(const KZGSettings *s, size_t max_batch, int caller_streams);

/* "Direct" fixed-base MSM for this settings object: trade HBM capacity for arithmetic. With every
 * multiple d * 2^(window_bits * j) * P_i of every setup point resident (window_bits 10 .. 16: 6, 11, 21, 36, 68,
 * 135, 240 GB with packed rows, 8/7 of that with the rows aligned to 128-byte lines, see lwkzg_direct_row_bytes), the 4096-term MSM behind every entry point above becomes 4096 * ceil(255 / window_bits) gathered
 * mixed additions (26, 24, 22, 20, 19, 17, 16 per scalar): no digit sort, no buckets, no bucket reduction. Results
 * are bit-identical between all widths and the bucket engine. window_bits = 0 frees the table and selects the bucket
 * engine (9 MB table, 20 additions per scalar plus sort and reduction).
 * Returns C_KZG_MALLOC (engine unchanged and still usable) when the table does not fit, C_KZG_BADARGS for
 * other widths. Replaces nothing in the reference: lambdaworks' pippenger::msm (call sites src/lib.rs:242,270,329,394)
 * has no precomputation at all.
 * What a load_trusted_setup* call selects by itself (for consumers that only know the nine reference symbols):
 *   LWKZG_DIRECT_BITS unset  the DEFAULT engine: the widest table of 13 .. 10 bits that takes at most a quarter of the
 *                            device memory free at load time (13 bits on an empty MI355X), else the bucket engine;
 *   LWKZG_DIRECT_BITS=0      the bucket engine;   =10..16  that width (bucket engine if it does not fit);
 *   LWKZG_DIRECT_BITS=auto   the widest of 16 .. 10 that fits. */
C_KZG_RET lwkzg_enable_direct_table(const KZGSettings *s, int window_bits);
int lwkzg_direct_table_bits(const KZGSettings *s);   /* 0 = bucket engine, 10..16 = direct table live, -1 = bad settings */
int lwkzg_direct_num_windows(int window_bits);       /* additions per scalar on the direct path (0 for other widths) */
/* The forms the live direct table(s) are in: bit 0 = monomial ([tau^i]G: reference mode, and every proof's quotient), bit 1 =
 * Lagrange ([l_i(tau)]G in the blob's own order: a c-kzg commitment is then an MSM over the blob's evaluations as they stand, no
 * transform -- SURVEY Appendix D; the reference left this conversion commented out, src/lib.rs:760-770, src/srs.rs:117-124).
 * The table is built in the form of the mode the settings answer in at that moment (lwkzg_enable_direct_table, the load's own
 * choice, lwkzg_settings_set_mode) and in the other form as well when that fits beside it with 8 GiB to spare (always up to 14 bits
 * on an empty MI355X, never at 15 / 16); the Lagrange form only once the settings have answered in c-kzg mode (a settings object that
 * merely follows the process default gets it at its first c-kzg call, and the second table then only within a quarter of the free
 * memory, the rule the load picks its own table by). No result depends on
 * it: without a Lagrange table a c-kzg commitment pays the inverse transform (k_ntt4096, +4 %); without a monomial table a c-kzg proof
 * pays one forward transform of its quotient, and reference mode runs on the monomial buckets. 0 = bucket engine, -1 = bad settings. */
int lwkzg_direct_table_forms(const KZGSettings *s);
/* lwkzg_enable_direct_table with the forms named: 1 = monomial only, 2 = Lagrange only (a consumer that only ever speaks c-kzg and wants
 * the widest table: 16 bits = 275 GB in ONE form), 3 = both or C_KZG_MALLOC. C_KZG_BADARGS for anything else. */
C_KZG_RET lwkzg_enable_direct_table_forms(const KZGSettings *s, int window_bits, int forms);
/* Bytes from one table row to the next: 128 when every row got a 128-byte line of its own (chosen whenever that table
 * leaves 8 GiB of the device free: one line per gather, +2.5 % / +5 % / +1.4 % at 13 / 15 / 16 bits), 112 when the rows are
 * packed (the sizes quoted above); 0 = bucket engine, -1 = bad settings. LWKZG_DIRECT_ROW=112|128 forces one. */
int lwkzg_direct_row_bytes(const KZGSettings *s);

/* The Fiat-Shamir challenges of device-resident blobs: z_i = compute_challenge(blob_i, commitment_i)
 * (src/utils.rs:120-154) as n x 32 bytes in the mode's byte order, canonical. This is the hash kernel of
 * lwkzg_compute_blob_kzg_proof_batch_device on its own (test / pipeline hook); the commitment bytes are hashed as given. */
C_KZG_RET lwkzg_compute_challenges_device(void *z32_dev, const void *blobs_dev, const void *commitments48_dev, size_t n,
                                          const KZGSettings *s, void *stream);

/* General G1 multi-scalar multiplication against the first `npoints` setup points:
 * scalars_dev = n_msm x npoints x 32 bytes (big-endian, reduced mod r), out = n_msm x 48 bytes compressed.
 * (reference: g1_lincomb, src/lib.rs:234-243, over srs.powers_main_group.) */
C_KZG_RET lwkzg_g1_lincomb_setup_device(void *out48_dev, const void *scalars_be_dev, size_t n_msm, const KZGSettings *s,
                                        void *stream);

/* Long MSM over the setup tiled end to end: out = sum_k scalars[k] * g1[k mod 4096], n_terms a positive multiple of
 * 4096 (e.g. 2^20), scalars big-endian 32-byte, device-resident; out = 48 bytes compressed (device pointer).
 * One fixed-base 4096-term MSM per tile plus one final sum. */
C_KZG_RET lwkzg_g1_msm_tiled_device(void *out48_dev, const void *scalars_be_dev, size_t n_terms, const KZGSettings *s,
                                    void *stream);
/* Host helper for sharded long MSMs: out = sum of n compressed G1 points (48 bytes each; infinity allowed). */
C_KZG_RET lwkzg_g1_sum_compressed(uint8_t out48[48], const uint8_t *points48, size_t n);

/* Batched Fr transform on device-resident data: n vectors of 4096 big-endian 32-byte elements,
 * natural order in and out; inverse != 0 scales by 4096^-1. */
C_KZG_RET lwkzg_fr_ntt4096_device(void *out_dev, const void *in_dev, size_t n, int inverse, const KZGSettings *s,
                                  void *stream);

/* Multi-GPU hand-off of a loaded setup (one process per GPU; rank 0 loads, the others import what an
 * RCCL broadcast delivered). The image is one contiguous DEVICE buffer. */
size_t lwkzg_setup_image_bytes(void);
C_KZG_RET lwkzg_setup_export_device(const KZGSettings *s, void *image_dev, void *stream);
C_KZG_RET lwkzg_setup_import_device(KZGSettings *out, const void *image_dev);

/* c-kzg-4844 trusted setups. load_trusted_setup* above read the G1 points as MONOMIAL powers [tau^i]G, which is
 * the reference's reading (src/srs.rs). c-kzg-4844 itself carries them in LAGRANGE form, natural order: its 1.x load_trusted_setup and
 * trusted_setup.txt hold only that form, its 2.x file and loader hold Lagrange G1, monomial G2, monomial G1. Handing such a file to
 * load_trusted_setup_file succeeds (4096 valid subgroup points) and every result afterwards is wrong; these three loaders are the way
 * in for it, and lwkzg_trusted_setup_check is the one call that tells a mis-loaded setup.
 * The result is a KZGSettings as load_trusted_setup builds from the matching monomial bytes (g1_values: the 4096 MONOMIAL points,
 * reference blst_fp convention; every call, free_trusted_setup and the setup image work on it), with two differences: it answers in
 * c-kzg mode from the start, as after lwkzg_settings_set_mode(s, LWKZG_MODE_CKZG) -- the table the load picks is built in the
 * Lagrange form first; another mode may be set afterwards --, and its Lagrange form is live at once, taken from the input.
 * A mainnet consumer calls lwkzg_settings_set_mode(&s, LWKZG_MODE_ETH) after the load; it is free (both modes run on the Lagrange form).
 * One-section form: the monomial points are derived on the device (4096 MSMs over the Lagrange points). Three-section form: nothing is
 * derived; both sections are validated and held against each other (a random polynomial committed over each: two MSMs), and the load
 * fails closed on a mismatch, which c-kzg itself does not check.
 * C_KZG_BADARGS (c-kzg's code, in both modes): a NULL pointer; counts other than 4096 / 65; a token that is not hex of the right
 * length or a token count that fits neither layout; a G1 point of either section that is not a compressed point of the subgroup or is
 * the point at infinity; a bad G2 point; a derived monomial point at infinity; two G1 sections that are not the same setup.
 * C_KZG_MALLOC: memory; C_KZG_ERROR: a failing device call, no GPU. On failure *out is untouched and nothing stays allocated;
 * lwkzg_last_error names the section and the index of a bad point. */
/* c-kzg-4844 1.x's load_trusted_setup: g1 = 4096 compressed LAGRANGE points [l_i(tau)]G1 in NATURAL order (l_i over w^i), g2 = 65 monomial */
C_KZG_RET lwkzg_load_trusted_setup_lagrange(KZGSettings *out, const uint8_t *g1_lagrange_bytes, size_t n1,
                                            const uint8_t *g2_bytes, size_t n2);
/* c-kzg-4844 2.x's load_trusted_setup (its argument order; `precompute` accepted and ignored: this library has its own tables) */
C_KZG_RET lwkzg_load_trusted_setup_ckzg(KZGSettings *out, const uint8_t *g1_monomial_bytes, size_t n_g1_monomial,
                                        const uint8_t *g1_lagrange_bytes, size_t n_g1_lagrange,
                                        const uint8_t *g2_monomial_bytes, size_t n_g2, uint64_t precompute);
/* either c-kzg text layout, told apart by the token count: "n1 n2", n1 Lagrange G1, n2 G2 [, n1 monomial G1]; tokens separated by ANY whitespace */
C_KZG_RET lwkzg_load_trusted_setup_file_ckzg(KZGSettings *out, FILE *in);
/* the Lagrange form of a loaded setup, 4096 x 48 bytes compressed, NATURAL order (what a c-kzg 1.x file holds); derives it if absent
 * (C_KZG_MALLOC, as lwkzg_settings_set_mode's derivation, when it cannot be had) */
C_KZG_RET lwkzg_setup_g1_lagrange(uint8_t *out, const KZGSettings *s);
/* is this a powers-of-tau setup? *ok = g1_values[0] and g2_values[0] are the generators, e(A, G2) e(-B, g2_values[1]) == 1 for
 * A = sum_(j<4095) rho^j g1_values[j+1], B = sum_(j<4095) rho^j g1_values[j] (rho hashed from the setup's bytes; two MSMs on the settings'
 * engine), and e(g1_values[1], g2_values[k]) e(-g1_values[0], g2_values[k+1]) == 1 for k < 64 (the host's pairing). For settings of any
 * loader, hand-built ones included; never changes them. C_KZG_OK with the verdict, C_KZG_BADARGS for NULL or bad settings. About 0.1 s. */
C_KZG_RET lwkzg_trusted_setup_check(bool *ok, const KZGSettings *s);

/* ONE process, SEVERAL GPUs (csrc/multi.hip): the node-level form of the batch entry points for the reference's own kind of caller
 * -- plain C calls, /root/reference/fuzz/base_fuzz.h:17-34, src/lib.rs:253-283 -- which has no torch.distributed. lwkzg_multi_load*
 * parses, validates and prepares the setup on devices[0] exactly as load_trusted_setup* does (src/lib.rs:709-802), delivers the
 * 10.3 MB setup image to the other devices device-to-device (hipMemcpyPeer: xGMI on an MI355X node) and lets every device build
 * its own MSM engine (all at once). The batch calls cut the batch into contiguous shards, blob k of n -> device floor(k G / n)
 * (SURVEY 8e), run each shard through the single-device entry point above on a host thread of its own, and write the results
 * in place: no reduction, no data-path collective. The batch verification is the reference's single check (ONE Fiat-Shamir r,
 * ONE linear combination, ONE pairing; src/lib.rs:639-692) via the lwkzg_verify_shard_* steps below. Bytes equal to the
 * single-device calls. A device ordinal may appear more than once (several contexts on one GPU: how the one-GPU tests run it).
 * lwkzg_multi_settings(m, k) is the k-th device's KZGSettings, for everything that is per device (lwkzg_reserve, timing, ...). */
typedef struct LwkzgMulti LwkzgMulti;
C_KZG_RET lwkzg_multi_load(LwkzgMulti **out, const uint8_t *g1_bytes, size_t n1, const uint8_t *g2_bytes, size_t n2, const int *devices,
                           size_t n_devices);
C_KZG_RET lwkzg_multi_load_file(LwkzgMulti **out, FILE *in, const int *devices, size_t n_devices);
void lwkzg_multi_free(LwkzgMulti *m);
size_t lwkzg_multi_device_count(const LwkzgMulti *m);
int lwkzg_multi_device(const LwkzgMulti *m, size_t k);                    /* ordinal of the k-th entry, -1 out of range */
const KZGSettings *lwkzg_multi_settings(const LwkzgMulti *m, size_t k);  /* NULL out of range */
C_KZG_RET lwkzg_multi_set_mode(const LwkzgMulti *m, int mode);           /* lwkzg_settings_set_mode on every device */
C_KZG_RET lwkzg_multi_enable_direct_table(const LwkzgMulti *m, int window_bits); /* every device at once; first failure returned */
C_KZG_RET lwkzg_multi_blob_to_kzg_commitment_batch(KZGCommitment *out, const Blob *blobs, size_t n, const LwkzgMulti *m, size_t *first_bad);
C_KZG_RET lwkzg_multi_compute_blob_kzg_proof_batch(KZGProof *out, const Blob *blobs, const Bytes48 *commitments, size_t n, const LwkzgMulti *m,
                                                   size_t *first_bad);
C_KZG_RET lwkzg_multi_compute_kzg_proof_batch(KZGProof *proofs_out, Bytes32 *ys_out, const Blob *blobs, const Bytes32 *zs, size_t n,
                                              const LwkzgMulti *m, size_t *first_bad);
C_KZG_RET lwkzg_multi_verify_blob_kzg_proof_batch(bool *ok, const Blob *blobs, const Bytes48 *commitments, const Bytes48 *proofs, size_t n,
                                                  const LwkzgMulti *m);
/* The same three calls for shards that are ALREADY in HBM: device k's shard is n_per_device[k] blobs behind blobs_dev[k] (a pointer
 * on device k), results in place behind out48_dev[k] (48 bytes per blob). Nothing crosses PCIe but verdicts and, for the
 * verification, the 160-byte records. first_bad counts through the shards in device order. Synchronous. */
C_KZG_RET lwkzg_multi_blob_to_kzg_commitment_batch_device(void *const *out48_dev, const void *const *blobs_dev, const size_t *n_per_device,
                                                          const LwkzgMulti *m, size_t *first_bad);
C_KZG_RET lwkzg_multi_compute_blob_kzg_proof_batch_device(void *const *out48_dev, const void *const *blobs_dev, const void *const *commitments48_dev,
                                                          const size_t *n_per_device, const LwkzgMulti *m, size_t *first_bad);
C_KZG_RET lwkzg_multi_verify_blob_kzg_proof_batch_device(bool *ok, const void *const *blobs_dev, const void *const *commitments48_dev,
                                                         const void *const *proofs48_dev, const size_t *n_per_device, const LwkzgMulti *m);
/* THE shard rule (multi.hip and lambdaworks_kzg_amd/dist.py both use this function): item i of n_items belongs to part
 * floor(i * parts / n_items); part k owns [*first, *first + *count) = [ceil(k n / parts), ceil((k + 1) n / parts)). */
C_KZG_RET lwkzg_shard_range(size_t n_items, size_t parts, size_t k, size_t *first, size_t *count);
/* BASELINE configs[4] over the devices: out = sum_k scalars[k] * g1[k mod 4096], n_terms a positive multiple of 4096, HOST-resident
 * big-endian scalars; whole tiles per device, one 48-byte partial sum back from each, added on the host. */
C_KZG_RET lwkzg_multi_g1_msm_tiled(uint8_t out48[48], const uint8_t *scalars_be, size_t n_terms, const LwkzgMulti *m);

/* verify_blob_kzg_proof_batch (src/lib.rs:525-614, 639-692) for a batch that is ALREADY on the device: blobs (n * 131072 bytes),
 * commitments and proofs (n * 48 each) are device pointers, produced on `stream` (a hipStream_t; NULL = already complete). The call
 * is synchronous, as the reference's: *ok is a host bool and the pairing check runs on the host; nothing but the 160-byte records
 * crosses PCIe. Same verdicts, return codes and empty-batch rule as verify_blob_kzg_proof_batch. */
C_KZG_RET lwkzg_verify_blob_kzg_proof_batch_device(bool *ok, const void *blobs_dev, const void *commitments48_dev, const void *proofs48_dev,
                                                   size_t n, const KZGSettings *s, void *stream);

/* verify_blob_kzg_proof_batch (src/lib.rs:525-692) for a batch SHARDED over several processes / GPUs, as the
 * reference computes it: ONE Fiat-Shamir scalar r over the whole batch (compute_r_powers, src/utils.rs:166-206), ONE
 * random linear combination, ONE pairing check. Rank k holds blobs [first_k, first_k + n_k) of the n_total:
 *   1. lwkzg_verify_shard_begin: per blob on this rank's GPU -- validate C_i and pi_i, z_i = compute_challenge,
 *      y_i = p_i(z_i); writes the shard's n_k transcript records (C 48 | z 32 | y 32 | pi 48 = 160 bytes each) and keeps
 *      the decompressed points on the device behind *shard_out;
 *   2. all-gather the records (160 bytes per blob; lambdaworks_kzg_amd/dist.py does it with torch.distributed);
 *   3. lwkzg_verify_shard_partial: r from ALL n_total records; this shard's terms of sum r^i pi_i, sum r^i z_i pi_i,
 *      sum r^i C_i (three affine points) and of sum r^i y_i (one scalar) -> LWKZG_VERIFY_PARTIAL_BYTES bytes;
 *   4. all-gather the partial sums; lwkzg_verify_shards_finish adds them and does the pairing check (on every rank, or
 *      on one).
 * verify_blob_kzg_proof_batch itself is steps 1, 3, 4 with one shard. Errors as there (invalid point / non-canonical
 * field element: C_KZG_ERROR in reference mode, C_KZG_BADARGS in c-kzg mode); n_total == 0 gives ok = false. A shard may
 * be empty (n_local = 0). Several shards may be open on one settings object (each owns its device scratch). */
#define LWKZG_VERIFY_RECORD_BYTES 160
#define LWKZG_VERIFY_PARTIAL_BYTES 328
typedef struct LwkzgVerifyShard LwkzgVerifyShard;
C_KZG_RET lwkzg_verify_shard_begin(LwkzgVerifyShard **shard_out, uint8_t *records_out /* n_local * 160 */, const Blob *blobs,
                                   const Bytes48 *commitments, const Bytes48 *proofs, size_t n_local, const KZGSettings *s);
/* Step 1 for a shard that is already in HBM: DEVICE pointers (produced on `stream`, NULL = already complete); records to the host. */
C_KZG_RET lwkzg_verify_shard_begin_device(LwkzgVerifyShard **shard_out, uint8_t *records_out /* n_local * 160, host */, const void *blobs_dev,
                                          const void *commitments48_dev, const void *proofs48_dev, size_t n_local, const KZGSettings *s,
                                          void *stream);
C_KZG_RET lwkzg_verify_shard_partial(uint8_t *partial_out /* 328 */, LwkzgVerifyShard *shard, const uint8_t *records_all /* n_total * 160 */,
                                     size_t n_total, size_t first_index);
void lwkzg_verify_shard_free(LwkzgVerifyShard *shard);
C_KZG_RET lwkzg_verify_shards_finish(bool *ok, const uint8_t *partials /* n_shards * 328 */, size_t n_shards, size_t n_total,
                                     const KZGSettings *s);

/* lwkzg_verify_blob_kzg_proof_batch_device without a parked host thread: a VERIFIER takes device-resident batches on the caller's
 * stream and answers each into a LwkzgVerifyResult, in stream order.
 *   lwkzg_verifier_new      allocates everything a call of up to max_blobs blobs needs (device scratch, pinned blocks, events, job slots;
 *                           the settings' workspace grows as a call of that size would grow it). The only call of the five that may
 *                           allocate or synchronise the device. C_KZG_BADARGS: NULL arguments, max_blobs == 0; C_KZG_MALLOC: no memory
 *                           (the settings stay usable).
 *   lwkzg_verifier_enqueue  the synchronous device call split where that call first waits: same inputs (device pointers produced on
 *                           `stream`, NULL = already complete), same mode resolution at entry, same verdict, return code and empty-batch
 *                           rule -- written to *result instead. It returns as soon as everything is enqueued: no wait for a stream or
 *                           an event, no allocation. *result is any host memory that stays valid until state == 1 (pinned mapped
 *                           memory lets a later kernel on the same stream read the verdict); state is 0 when the call returns and is
 *                           stored LAST, with release order. Work enqueued on `stream` AFTER the call is ordered behind the verdict.
 *                           The inputs must stay untouched until the call completes. The call's own return value covers only what is
 *                           known at once -- C_KZG_BADARGS: NULL v or result, n above the verifier's capacity, NULL inputs with n > 0, a
 *                           verifier whose settings were freed; C_KZG_ERROR: a failing enqueue -- and *result is then completed on the
 *                           spot with that code. n == 0 completes on the spot with the mode's empty-batch verdict. A rejected input
 *                           is an answer: the call returns C_KZG_OK, result->rc is the mode's code and first_bad the lowest such index.
 *                           Calls on ONE verifier run one after the other on the GPU (they share its scratch, ordered by events); up
 *                           to LWKZG_VERIFIER_DEPTH may be in flight, and ONE MORE WAITS FOR THE OLDEST TO COMPLETE: the only place this
 *                           call waits for the GPU. Like every device-resident call it takes the settings' context lock while it
 *                           enqueues, and a SYNCHRONOUS call on the same settings holds that lock until its own GPU work is done: an
 *                           enqueue issued meanwhile by another thread waits for that call. Calls on TWO verifiers on two caller
 *                           streams run on the settings' two contexts. Call lwkzg_reserve_streams(s, n, 2) BEFORE lwkzg_verifier_new:
 *                           otherwise the first enqueue that finds the first context busy creates the second one (an allocation
 *                           inside enqueue), and a second context created after lwkzg_verifier_new grows its workspace inside the
 *                           first enqueue that lands on it. Synchronous verifications on the same settings stay correct meanwhile.
 *   lwkzg_verifier_pending  calls enqueued and not yet complete; -1 for a NULL handle.
 *   lwkzg_verifier_wait     until pending == 0.
 *   lwkzg_verifier_free     waits first; NULL is fine. free_trusted_setup on settings that still have verifiers waits for their calls in
 *                           flight; such a verifier answers C_KZG_BADARGS to further enqueues and is still freed with this call.
 * Not covered: host-pointer batches (they are upload-bound), lwkzg_multi_*, the per-item verifications, and stream capture -- enqueue on
 * a capturing stream is not supported. The cell proof batch has a verifier of its own: lwkzg_cell_verifier_* below, which groups the
 * commitments on the GPU instead of de-duplicating them on the host mid-call. With the experiment arm LWKZG_VERIFY_MSM=0 the
 * enqueue runs the synchronous call and completes *result before it returns (first_bad is then not reported). */
#define LWKZG_VERIFIER_DEPTH 4
typedef struct {
    int32_t  state;      /* 0 = pending, 1 = complete; written LAST, with release order */
    int32_t  rc;         /* the C_KZG_RET the synchronous device call would have returned */
    int32_t  ok;         /* 0 / 1: its *ok */
    uint32_t first_bad;  /* lowest rejected index, 0xffffffff = none */
    uint8_t  r[32];      /* the batch challenge, canonical big-endian, as lwkzg_batch_challenge_host writes it */
    uint8_t  partial[LWKZG_VERIFY_PARTIAL_BYTES]; /* as lwkzg_verify_shard_partial(first_index = 0) writes it */
} LwkzgVerifyResult;
typedef struct LwkzgVerifier LwkzgVerifier;
C_KZG_RET lwkzg_verifier_new(LwkzgVerifier **out, const KZGSettings *s, size_t max_blobs);
C_KZG_RET lwkzg_verifier_enqueue(LwkzgVerifier *v, LwkzgVerifyResult *result, const void *blobs_dev,
                                 const void *commitments48_dev, const void *proofs48_dev, size_t n, void *stream);
int       lwkzg_verifier_pending(const LwkzgVerifier *v);   /* calls enqueued and not yet complete, -1 = bad handle */
C_KZG_RET lwkzg_verifier_wait(LwkzgVerifier *v);            /* until pending == 0 */
void      lwkzg_verifier_free(LwkzgVerifier *v);            /* waits first; NULL is fine */
/* Host-only test hook: the two host steps of an enqueue back to back on caller-supplied blocks -- the n records, the lowest rejected
 * index (0xffffffff: none), the three sums (flag 1 | x 48 | y 48 each, as in a partial) and sum r^i y_i (canonical big-endian) -- with
 * the generator and the G2 points of *s. No GPU, no context; *out is complete when it returns. */
C_KZG_RET lwkzg_verifier_host_steps(LwkzgVerifyResult *out, const uint8_t *records, size_t n, uint32_t first_bad, const uint8_t *sums3x97,
                                    const uint8_t *ysum32, const KZGSettings *s, int mode);

/* Per-item verification: n independent verify_blob_kzg_proof calls (src/lib.rs:456-505) in one. For every i, ok_out[i] (0/1) and
 * rc_out[i] (a C_KZG_RET) are exactly what verify_blob_kzg_proof(&ok, &blobs[i], &commitments[i], &proofs[i], s) gives, in the mode the
 * settings answer in. A bad item is an answer, not a failure: the call returns C_KZG_OK once every item is decided, C_KZG_BADARGS for
 * NULL pointers, C_KZG_MALLOC / C_KZG_ERROR only when the device work itself fails. n == 0: C_KZG_OK, nothing written. Synchronous, like
 * lwkzg_verify_blob_kzg_proof_batch_device. Every step runs on the GPU, the pairing check of each item included.
 * Verify a batch with verify_blob_kzg_proof_batch first; this call is for a batch that answered false, or where every item needs its
 * own answer. */
C_KZG_RET lwkzg_verify_blob_kzg_proof_each(uint8_t *ok_out, int32_t *rc_out, const Blob *blobs, const Bytes48 *commitments,
                                           const Bytes48 *proofs, size_t n, const KZGSettings *s);
/* the same for inputs already in HBM (device pointers produced on `stream`, NULL = already complete); the verdicts come to the host */
C_KZG_RET lwkzg_verify_blob_kzg_proof_each_device(uint8_t *ok_out, int32_t *rc_out, const void *blobs_dev,
                                                  const void *commitments48_dev, const void *proofs48_dev, size_t n,
                                                  const KZGSettings *s, void *stream);
/* n independent verify_kzg_proof calls (src/lib.rs:407-453): item i is (commitments[i], zs[i], ys[i], proofs[i]); same contract */
C_KZG_RET lwkzg_verify_kzg_proof_each(uint8_t *ok_out, int32_t *rc_out, const Bytes48 *commitments, const Bytes32 *zs,
                                      const Bytes32 *ys, const Bytes48 *proofs, size_t n, const KZGSettings *s);
/* the same for openings already in HBM (device pointers produced on `stream`, NULL = already complete); the verdicts come to the host */
C_KZG_RET lwkzg_verify_kzg_proof_each_device(uint8_t *ok_out, int32_t *rc_out, const void *commitments48_dev, const void *zs32_dev,
                                             const void *ys32_dev, const void *proofs48_dev, size_t n, const KZGSettings *s, void *stream);

/* Batch verification of n openings (C_i, z_i, y_i, pi_i) with ONE pairing check: the consensus specs' verify_kzg_proof_batch, the inner
 * function of the reference's blob batch (src/lib.rs:639-692). Verify a batch with this call first and ask lwkzg_verify_kzg_proof_each
 * only when it answers false. In the mode the settings answer in, resolved at entry:
 *   validation  item i is valid exactly when verify_kzg_proof on it returns C_KZG_OK: C_i and pi_i by that call's rules for compressed
 *               G1 points (the infinity encodings it accepts included), z_i and y_i by the mode's scalar rule (reference mode: reduced;
 *               c-kzg and eth mode: rejected when not below r).
 *   record      canon(C_i) 48 | z_i 32 | y_i 32 | canon(pi_i) 48 = LWKZG_VERIFY_RECORD_BYTES, the layout lwkzg_verify_shard_begin
 *               writes: the points in their canonical encoding, z and y canonical in the mode's byte order (reference mode: the
 *               reduced value).
 *   challenge   r = lwkzg_batch_challenge_host(records, n, mode); the sums start at r^0.
 *   verdict     e(sum r^i C_i - [sum r^i y_i]G + sum r^i z_i pi_i, G2) e(-sum r^i pi_i, [tau]G2) == 1.
 *   codes       C_KZG_BADARGS for ok == NULL; other NULL arguments as verify_blob_kzg_proof_batch answers them. Any invalid item: the
 *               mode's code (C_KZG_ERROR in reference mode, C_KZG_BADARGS in c-kzg and eth mode) with *ok = false, and
 *               lwkzg_last_error names the lowest such index. n == 0: the mode's empty-batch verdict, decided before any device work.
 *               C_KZG_MALLOC / C_KZG_ERROR otherwise only when the device work itself fails.
 * For n == 1 the answer is verify_kzg_proof's. On the four columns of the records lwkzg_verify_shard_begin returns for a blob batch
 * the call has that batch's r, the partial of lwkzg_verify_shard_partial(first_index = 0) and verify_blob_kzg_proof_batch's verdict.
 * The host form uploads 160 bytes per item into the settings' grow-only verify scratch (no allocation once that has grown) and runs
 * the device path. */
C_KZG_RET lwkzg_verify_kzg_proof_batch(bool *ok, const Bytes48 *commitments, const Bytes32 *zs, const Bytes32 *ys,
                                       const Bytes48 *proofs, size_t n, const KZGSettings *s);
/* the same for openings already in HBM: device pointers, 16-byte aligned (a misaligned pointer is C_KZG_BADARGS, decided on the host),
 * produced on `stream` (NULL = already complete). Synchronous, *ok is a host bool, as lwkzg_verify_blob_kzg_proof_batch_device; only
 * the 160-byte records and the three sums cross PCIe. */
C_KZG_RET lwkzg_verify_kzg_proof_batch_device(bool *ok, const void *commitments48_dev, const void *zs32_dev, const void *ys32_dev,
                                              const void *proofs48_dev, size_t n, const KZGSettings *s, void *stream);
/* test hook, by the verdict call's own code path up to the pairing: r canonical big-endian as lwkzg_batch_challenge_host writes it,
 * partial as lwkzg_verify_shard_partial(first_index = 0) writes it; arguments and codes as the host call; n == 0 writes nothing */
C_KZG_RET lwkzg_verify_kzg_proof_batch_partial(uint8_t r_out[32], uint8_t partial_out[LWKZG_VERIFY_PARTIAL_BYTES],
                                               const Bytes48 *commitments, const Bytes32 *zs, const Bytes32 *ys,
                                               const Bytes48 *proofs, size_t n, const KZGSettings *s);
/* lwkzg_verify_kzg_proof_batch_device on a verifier (lwkzg_verifier_new above; its max_blobs counts openings for this call), with
 * lwkzg_verifier_enqueue's contract line by line: it returns once everything is enqueued, waits for nothing and allocates nothing;
 * state is stored last; rc, ok, first_bad, r and partial are what the synchronous call and the hook above define; a rejected input is
 * an answer (rc the mode's code, first_bad the lowest such index, the partial zero) and nothing behind r runs on unvalidated points; up
 * to LWKZG_VERIFIER_DEPTH calls may be in flight; n above the capacity, NULL or misaligned inputs and n == 0 complete on the spot; with
 * LWKZG_VERIFY_MSM=0 the call completes before it returns. Blob and opening calls may be mixed on one verifier and complete in order. */
C_KZG_RET lwkzg_verifier_enqueue_openings(LwkzgVerifier *v, LwkzgVerifyResult *result, const void *commitments48_dev,
                                          const void *zs32_dev, const void *ys32_dev, const void *proofs48_dev, size_t n, void *stream);

/* EIP-7594 (PeerDAS) cells and cell proofs. The blob stands for the polynomial p the settings' mode reads (reference mode: big-endian
 * coefficients reduced mod r; c-kzg mode: little-endian evaluations on the bit-reversed 4096 domain, each < r). With w = 7^((r-1)/8192)
 * and the extended domain D[j] = w^bitrev13(j), cell k (k < 128) holds p(D[64 k + t]) for t < 64, 32 bytes each in the mode's byte
 * order: cells 0 .. 63 are the evaluations on the 4096 domain (in c-kzg mode, the blob's own bytes), cells 64 .. 127 those of
 * p(w X). Proof k is [q_k(tau)]G1 compressed, q_k = p div (X^64 - c_k) with c_k = D[64 k]^64: the quotient by the vanishing
 * polynomial of cell k's coset. DESIGN.md section 4h. */
#ifndef FIELD_ELEMENTS_PER_EXT_BLOB
#define FIELD_ELEMENTS_PER_EXT_BLOB (2 * FIELD_ELEMENTS_PER_BLOB)
#endif
#ifndef FIELD_ELEMENTS_PER_CELL
#define FIELD_ELEMENTS_PER_CELL 64
#endif
#ifndef CELLS_PER_EXT_BLOB
#define CELLS_PER_EXT_BLOB (FIELD_ELEMENTS_PER_EXT_BLOB / FIELD_ELEMENTS_PER_CELL)
#endif
#ifndef BYTES_PER_CELL
#define BYTES_PER_CELL (FIELD_ELEMENTS_PER_CELL * BYTES_PER_FIELD_ELEMENT)
#endif
typedef struct { uint8_t bytes[BYTES_PER_CELL]; } Cell;
/* The 128 cells and 128 proofs of one blob (c-kzg-4844 2.x's argument order). Either output may be NULL: with proofs == NULL only the
 * cells are computed and no MSM runs; both NULL is an argument error. Synchronous. */
C_KZG_RET lwkzg_compute_cells_and_kzg_proofs(Cell *cells, KZGProof *proofs, const Blob *blob, const KZGSettings *s);
/* n blobs: cells and proofs are n x 128 each. The return code as the other host batches: a c-kzg-mode blob with an element >= r fails
 * the call (C_KZG_BADARGS; first_bad, if given, gets its index) and nothing is written. n == 0: C_KZG_OK, nothing written. */
C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_batch(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n, const KZGSettings *s,
                                                   size_t *first_bad);
/* the same on device pointers (cells_dev: n x 128 x 2048 bytes, proofs48_dev: n x 128 x 48 bytes, either NULL), asynchronous on `stream`
 * (NULL = the context's own). status_dev (optional): one word per blob, 0 or the mode's rejection code; a good blob's outputs are correct
 * whatever its neighbours' status. A call of 8 blobs or more fills whole MSM launch sets. */
C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_batch_device(void *cells_dev, void *proofs48_dev, const void *blobs_dev, size_t n,
                                                          const KZGSettings *s, void *stream, int32_t *status_dev);

/* Chosen columns only: the cells and proofs of columns[0 .. num_columns) of n blobs, blob-major and compact --
 * cells[b * num_columns + i] and proofs[b * num_columns + i] are byte for byte cells[128 b + columns[i]] and proofs[128 b + columns[i]] of
 * lwkzg_compute_cells_and_kzg_proofs_batch on the same blobs and settings, in every mode, on every MSM engine and on either cell proof
 * engine; with all 128 columns the call is that call. columns is a HOST array: num_columns in 1 .. 128, every index below 128, strictly
 * ascending (the rule cell_indices follows). Either output may be NULL; with proofs == NULL no MSM runs. On the MSM engine a proof is one
 * 4096-term MSM, so the call costs about num_columns / 128 of the full one; with the FK20 engine on, that engine serves the call when
 * n * num_columns >= 128 * min_blobs (as many MSMs as a full call at the threshold brings) and the MSM engine below.
 * C_KZG_BADARGS in both modes, decided before any device work: s NULL; with n > 0 blobs NULL, both outputs NULL, columns NULL, num_columns 0
 * or above 128, an index of 128 or more, a list not strictly ascending. A c-kzg-mode blob with an element >= r fails the call with the
 * mode's code (first_bad, if given, gets its index) and nothing is written, as in the full call. n == 0: C_KZG_OK, nothing written,
 * whatever the other pointers are. Synchronous. */
C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_columns(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n, const uint64_t *columns,
                                                     size_t num_columns, const KZGSettings *s, size_t *first_bad);
/* the same on device pointers (cells_dev: n x num_columns x 2048 bytes, proofs48_dev: n x num_columns x 48 bytes, either NULL),
 * asynchronous on `stream` (NULL = the context's own); columns stays a HOST array, read before the call returns and handed to the kernels
 * by value: calls with different lists may follow each other on one stream with no synchronisation between them. status_dev (optional):
 * one word per blob, 0 or the mode's rejection code; a good blob's outputs are correct whatever its neighbours' status. A call of
 * 1024 / num_columns blobs or more fills whole MSM launch sets (lwkzg_reserve: 1024 covers every column call). */
C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_columns_device(void *cells_dev, void *proofs48_dev, const void *blobs_dev, size_t n,
                                                            const uint64_t *columns /* HOST */, size_t num_columns, const KZGSettings *s,
                                                            void *stream, int32_t *status_dev);

/* EIP-7594 recover_cells_and_kzg_proofs: all 128 cells and all 128 proofs of a blob from num_cells of its cells, 64 <= num_cells <= 128.
 * cells[i] is cell cell_indices[i], in the settings' mode's byte order; the indices are below 128 and strictly ascending (c-kzg-4844 2.x's
 * rule and argument order). With p the polynomial of degree < 4096 that takes the given values on the given cells' cosets -- unique if it
 * exists -- the outputs are byte for byte what lwkzg_compute_cells_and_kzg_proofs returns for the blob that stands for p in the
 * settings' mode. Either output may be NULL (proofs NULL: no MSM runs). DESIGN.md section 4j.
 * C_KZG_BADARGS in both modes, decided before any device work: s NULL; cell_indices or cells NULL; both outputs NULL; num_cells outside
 * 64 .. 128; an index of 128 or more; indices not strictly ascending. A bad input -- a cell element that is not below r (never reduced, not
 * in reference mode either), or cells that no polynomial of degree < 4096 goes through (possible from 65 cells on; with exactly 64 every
 * canonical input is consistent, and with 128 the call is a consistency check plus the proofs) -- gives the mode's code for it
 * (C_KZG_ERROR in reference mode, C_KZG_BADARGS in c-kzg mode) and nothing is written. Synchronous. */
C_KZG_RET lwkzg_recover_cells_and_kzg_proofs(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                             const Cell *cells, size_t num_cells, const KZGSettings *s);
/* n blobs that share ONE index set (the rows of a block seen through the same columns: what a reconstructing node holds).
 * cells: n x num_cells x 2048 bytes, blob-major; outputs n x 128 each, either may be NULL (proofs NULL: no MSM runs). A bad blob fails
 * the call with the mode's code (first_bad, if given, gets its index) and nothing is written. n == 0: C_KZG_OK, nothing written. */
C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_batch(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                                   const Cell *cells, size_t num_cells, size_t n, const KZGSettings *s, size_t *first_bad);
/* cells_dev / outputs are DEVICE pointers (16-byte aligned), cell_indices stays a HOST array (at most 128 words, read before the call
 * returns); asynchronous on `stream` (NULL = the context's own); status_dev optional, one word per blob: 0 or the mode's code for a bad
 * input; a good blob's outputs are correct whatever its neighbours' status. No allocation and no device synchronisation once
 * lwkzg_reserve has covered the batch (8 blobs' worth of proofs = 1024, or 2 slots per blob without proofs). */
C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_batch_device(void *recovered_cells_dev, void *recovered_proofs48_dev,
                                                          const uint64_t *cell_indices, const void *cells_dev, size_t num_cells, size_t n,
                                                          const KZGSettings *s, void *stream, int32_t *status_dev);

/* Chosen columns only: n blobs through ONE index set, as lwkzg_recover_cells_and_kzg_proofs_batch takes them, and
 * of the result the cells and proofs of columns[0 .. num_columns) alone, blob-major and compact: cells_out[b * num_columns + i] and
 * proofs_out[b * num_columns + i] are byte for byte entries 128 b + columns[i] of that call's outputs -- what a node that has just
 * reconstructed a block needs to re-seed the columns it lacks (pass the complement of cell_indices). columns as in
 * lwkzg_compute_cells_and_kzg_proofs_columns; it may name given columns too (their cells come back as given). Argument errors
 * (C_KZG_BADARGS in both modes, before any device work) are those of the full call plus those of the list; a bad blob -- an element not
 * below r, inconsistent cells: the check does not depend on columns -- fails the call with the mode's code (first_bad, if given, gets its
 * index) and nothing is written. n == 0: C_KZG_OK, nothing written. Either output may be NULL (proofs_out NULL: no MSM runs).
 * Synchronous. The _mixed forms have no column variant. */
C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_columns(Cell *cells_out, KZGProof *proofs_out, const uint64_t *cell_indices, const Cell *cells,
                                                     size_t num_cells, size_t n, const uint64_t *columns, size_t num_columns,
                                                     const KZGSettings *s, size_t *first_bad);
/* the same on device pointers (16-byte aligned; outputs n x num_columns x 2048 and n x num_columns x 48 bytes), cell_indices and columns
 * HOST arrays read before the call returns; asynchronous on `stream`; status_dev as in lwkzg_recover_cells_and_kzg_proofs_batch_device. */
C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_columns_device(void *cells_out_dev, void *proofs48_out_dev, const uint64_t *cell_indices,
                                                            const void *cells_dev, size_t num_cells, size_t n,
                                                            const uint64_t *columns /* HOST */, size_t num_columns, const KZGSettings *s,
                                                            void *stream, int32_t *status_dev);

/* n blobs, each seen through an index set of its OWN (the rows of several blocks, each block through the columns that reached the node: a
 * node catching up, a backfill, a supernode reconstructing for its peers). num_cells[b] is blob b's count, 64 .. 128; cell_indices
 * holds the blobs' index lists one after the other and cells their cells in the same order, num_cells[0] + .. + num_cells[n - 1] entries
 * each; outputs n x 128 each, either may be NULL (proofs NULL: no MSM runs). For every blob b the outputs and its contribution to the
 * return code are byte for byte those of lwkzg_recover_cells_and_kzg_proofs on (its list, its cells, num_cells[b]) alone, in the mode
 * the settings answer in and on every cell proof engine; the FK20 threshold counts this call's n. Lists that name the same cells share
 * one table on the device, so n blobs of a few blocks cost a few tables. DESIGN.md section 4j.
 * C_KZG_BADARGS in both modes, decided before any device work: s NULL; with n > 0 cell_indices, cells or num_cells NULL; both outputs
 * NULL; a count outside 64 .. 128; an index of 128 or more; a list not strictly ascending -- where one blob's list is at fault,
 * first_bad (if given) gets that blob's index. A bad blob (an element not below r, inconsistent cells) fails the call with the mode's
 * code (first_bad, if given, gets its index) and nothing is written. n == 0: C_KZG_OK, nothing written, whatever the other pointers
 * are. Synchronous. */
C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_mixed(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                                   const Cell *cells, const size_t *num_cells, size_t n, const KZGSettings *s,
                                                   size_t *first_bad);
/* cells_dev / outputs are DEVICE pointers (16-byte aligned), cell_indices and num_cells stay HOST arrays (read before the call returns);
 * asynchronous on `stream` (NULL = the context's own); status_dev optional, one word per blob: 0 or the mode's code for a bad input; a
 * good blob's outputs are correct whatever its neighbours' status. Calls that follow each other on one stream need no synchronisation
 * between them: the sets reach the kernels as launch arguments and through a device block that only kernels of the call write, in
 * stream order. That block belongs to the settings object and only grows: a call with more DISTINCT sets than any mixed call on these
 * settings before it (the first 64 come with the first call) waits for the device, frees the block and allocates one of twice the
 * size, about 16 KiB per set; up to that count no later call allocates or synchronises, once lwkzg_reserve has covered the batch as for
 * lwkzg_recover_cells_and_kzg_proofs_batch_device. */
C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_mixed_device(void *recovered_cells_dev, void *recovered_proofs48_dev,
                                                          const uint64_t *cell_indices, const void *cells_dev, const size_t *num_cells,
                                                          size_t n, const KZGSettings *s, void *stream, int32_t *status_dev);

/* EIP-7594 verify_cell_kzg_proof_batch: do the n items (commitments[i], cell_indices[i], cells[i], proofs[i]) belong together?
 * c-kzg-4844 2.x's argument order; the same commitment may appear many times and an item may repeat. cells are in the settings' mode's
 * byte order, as lwkzg_compute_cells_and_kzg_proofs writes them. DESIGN.md section 4i has the definition: commitments de-duplicated by
 * byte equality in order of first occurrence (m rows), a two-level transcript
 *     d_i = SHA-256(le64(row_i) | le64(k_i) | cell_i | proof_i)                                    (on the GPU, one hash per cell)
 *     r   = SHA-256("RCKZGCBATCH__V1_" | le64(4096) | le64(64) | le64(m) | le64(n) | the m distinct commitments | d_0 .. d_(n-1))
 * read in the mode's byte order and reduced (this transcript is the library's own in EVERY mode, LWKZG_MODE_ETH included: there only
 * the reading of the digest into r, and the r bytes of lwkzg_cell_verify_partials, are the mode's -- big-endian; the consensus specs'
 * single sequential hash over n x 2112 bytes would put milliseconds of serial SHA-256 in front of the sums, and the verdict does not
 * depend on the transcript), and one pairing check e(RLC - RLI + RLP, G2) e(-P, g2_values[64]) == 1 over
 * P = sum r^i pi_i, RLP = sum r^i c_(k_i) pi_i, RLC = sum_j (sum_(row_i = j) r^i) C_j and RLI = [sum r^i I_i(tau)]G1 (I_i: the
 * interpolant of cell i on its coset). The settings must carry all 65 G2 points.
 * Returns: C_KZG_BADARGS for ok == NULL, NULL pointers with n > 0 or an index >= 128 (decided on the host before any device work); the
 * mode's code for a bad input (C_KZG_ERROR in reference mode, C_KZG_BADARGS in c-kzg mode) when a distinct commitment or a proof is
 * not a compressed point of G1 (infinity allowed) or a cell element is not below r -- cell elements are never reduced, not in
 * reference mode either: cells are this library's own outputs and always canonical. *ok is false on every error.
 * n == 0: C_KZG_OK with *ok = true in BOTH modes (the consensus specs' and c-kzg-4844 2.x's rule for cells) -- unlike
 * verify_blob_kzg_proof_batch, whose empty batch answers false in reference mode.
 * Batch the columns of a slot into one call: the call's cost is mostly fixed. */
C_KZG_RET lwkzg_verify_cell_kzg_proof_batch(bool *ok, const Bytes48 *commitments, const uint64_t *cell_indices, const Cell *cells,
                                            const Bytes48 *proofs, size_t n, const KZGSettings *s);
/* the same for inputs already in HBM (16-byte aligned; produced on `stream`, NULL = the context's own); synchronous, *ok is a host bool,
 * as lwkzg_verify_blob_kzg_proof_batch_device. The cells stay on the device: the commitments and the indices come down, the row and
 * column lists go up, the digests and the status words come down. */
C_KZG_RET lwkzg_verify_cell_kzg_proof_batch_device(bool *ok, const void *commitments48_dev, const void *cell_indices_dev,
                                                   const void *cells_dev, const void *proofs48_dev, size_t n, const KZGSettings *s,
                                                   void *stream);
/* r and the four sums of the check, for tests and for a later sharded form, by the verdict call's own code path up to the pairing:
 * out = r 32 (the mode's byte order) | P | RLC | RLI | RLP, each flag 1 (1 = infinity) | x 48 | y 48 big-endian. Host arguments and
 * return codes as lwkzg_verify_cell_kzg_proof_batch; n == 0 writes nothing. */
#define LWKZG_CELL_VERIFY_PARTIAL_BYTES (32 + 4 * 97)
C_KZG_RET lwkzg_cell_verify_partials(uint8_t *out, const Bytes48 *commitments, const uint64_t *cell_indices, const Cell *cells,
                                     const Bytes48 *proofs, size_t n, const KZGSettings *s);
/* the transcript alone, on the host (no GPU, no settings): r_out = the challenge of the batch in `mode`'s byte order. NULL pointers with
 * n > 0, an index >= 128 or an unknown mode: C_KZG_BADARGS. */
C_KZG_RET lwkzg_cell_batch_challenge_host(uint8_t r_out[32], const Bytes48 *commitments, const uint64_t *cell_indices, const Cell *cells,
                                          const Bytes48 *proofs, size_t n, int mode);

/* lwkzg_verify_cell_kzg_proof_batch_device without a parked host thread: a CELL VERIFIER takes device-resident cell batches on the
 * caller's stream and answers each into a LwkzgCellVerifyResult, in stream order. The contract is
 * lwkzg_verifier_*'s above, line by line; what differs is said here.
 *   lwkzg_cell_verifier_new      allocates everything a call of up to max_cells items needs: a device block (the batch's buffers and the
 *                                grouping's table of at least 2 max_cells slots), a pinned block, events, job slots, the settings'
 *                                workspace for one MSM slot; copies g2_values[0] and g2_values[64] (the settings must carry all 65 G2
 *                                points); draws the 64-bit seed of the grouping's slot hash; derives the Lagrange form when the settings
 *                                answer in c-kzg mode. The only call of the five that may allocate or synchronise the device.
 *                                C_KZG_BADARGS: NULL arguments, max_cells == 0, settings without g2_values; C_KZG_MALLOC: no memory.
 *   lwkzg_cell_verifier_enqueue  the synchronous device call's inputs (device pointers, 16-byte aligned, produced on `stream`; NULL =
 *                                already complete), verdict, codes and precedence -- written to *result. It returns once everything is
 *                                enqueued: no wait for a stream or an event, no allocation (a settings object switched to c-kzg mode
 *                                AFTER lwkzg_cell_verifier_new derives its Lagrange form inside the first enqueue). The commitments are
 *                                never brought to the host to be grouped: rows, m and the row and column lists are made by kernels.
 *                                    any index >= 128       result->rc C_KZG_BADARGS in both modes, decided first whatever else is
 *                                                           wrong; first_bad the lowest such item
 *                                    a proof or a distinct commitment that is not a compressed point of G1 (infinity allowed), a cell
 *                                    element not below r    result->rc the mode's code (C_KZG_ERROR reference, C_KZG_BADARGS c-kzg);
 *                                                           first_bad the lowest item whose own cell, proof or commitment is at fault
 *                                                           (a bad commitment counts at the item it was first seen at)
 *                                    otherwise              result->rc C_KZG_OK, ok the verdict, m the number of distinct commitments,
 *                                                           partials exactly as lwkzg_cell_verify_partials writes them
 *                                A rejected batch is an answer: the call returns C_KZG_OK, and nothing behind r runs on its unvalidated
 *                                points or unchecked indices (partials are then zero). n == 0 completes on the spot with ok = 1 in BOTH
 *                                modes. Argument and capacity errors (NULL v or result, n above max_cells, NULL inputs with n > 0, freed
 *                                settings) complete *result on the spot with C_KZG_BADARGS, a failing enqueue with C_KZG_ERROR, and are
 *                                the call's return value. Up to LWKZG_VERIFIER_DEPTH calls may be in flight per verifier; ONE MORE WAITS
 *                                FOR THE OLDEST. Context lock, two verifiers on two streams, lwkzg_reserve_streams first: as above.
 *   lwkzg_cell_verifier_pending / _wait / _free   as lwkzg_verifier_pending / _wait / _free; free_trusted_setup waits for the calls in
 *                                flight of the settings' cell verifiers too.
 * Not covered: host-pointer batches, the per-item form, stream capture. The per-group form is lwkzg_cell_verifier_enqueue_groups
 * below, which gives the fields of LwkzgCellVerifyResult meanings of its own. */
typedef struct {
    int32_t  state;      /* 0 = pending, 1 = complete; written LAST, with release order */
    int32_t  rc;         /* the C_KZG_RET the synchronous device call would have returned */
    int32_t  ok;         /* 0 / 1: its *ok */
    uint32_t first_bad;  /* lowest item at fault, 0xffffffff = none */
    uint32_t m;          /* distinct commitments (0 when the call completed on the spot) */
    uint8_t  partials[LWKZG_CELL_VERIFY_PARTIAL_BYTES]; /* as lwkzg_cell_verify_partials writes them; zero unless rc == C_KZG_OK */
} LwkzgCellVerifyResult;
typedef struct LwkzgCellVerifier LwkzgCellVerifier;
C_KZG_RET lwkzg_cell_verifier_new(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_cells);
C_KZG_RET lwkzg_cell_verifier_enqueue(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, const void *commitments48_dev,
                                      const void *cell_indices_dev, const void *cells_dev, const void *proofs48_dev, size_t n, void *stream);
int       lwkzg_cell_verifier_pending(const LwkzgCellVerifier *v);   /* calls enqueued and not yet complete, -1 = bad handle */
C_KZG_RET lwkzg_cell_verifier_wait(LwkzgCellVerifier *v);            /* until pending == 0 */
void      lwkzg_cell_verifier_free(LwkzgCellVerifier *v);            /* waits first; NULL is fine */
/* Host-only test hook: the two host steps of an enqueue back to back on caller-supplied blocks, with the G2 points of *s. No GPU, no
 * context; *out is complete when it returns. distinct48: the m distinct commitments; digests32: the n per-cell digests; bad_index: the
 * lowest item with an index >= 128 (0xffffffff: none); status: 2 n fault words -- [i] item i's own (a cell element, its proof),
 * [n + j] distinct commitment j's; first_item: m words; sums3x97: P | RLP | RLC in the device's order (flag 1 | x 48 | y 48 each);
 * rli48: the interpolant's commitment, compressed. A rejected batch reads nothing behind what decides it. */
C_KZG_RET lwkzg_cell_verifier_host_steps(LwkzgCellVerifyResult *out, const uint8_t *distinct48, size_t m, const uint8_t *digests32, size_t n,
                                         uint32_t bad_index, const int32_t *status, const uint32_t *first_item, const uint8_t *sums3x97,
                                         const uint8_t *rli48, const KZGSettings *s, int mode);
/* Test hook: the grouping kernels alone on device inputs (n commitments of 48 bytes, n uint64 indices; the current device), every output
 * brought to host arrays: rows n, *m_out, distinct48 48 n (the m distinct commitments in order of first occurrence, then infinity
 * encodings), first_item n (m used), perm_row n / row_off n + 1 (m + 1 used), perm_col n / col_off 129, *bad_index (the lowest i with an
 * index >= 128, 0xffffffff: none; such items are in no column). The order inside a group of perm_row / perm_col is not defined. seed:
 * of the keyed slot hash; hash_mask is ANDed with the hash (0xffffffff in a verifier; 0 puts every key on one probe chain).
 * Synchronous. C_KZG_BADARGS: NULL pointers, n == 0; C_KZG_ERROR: the kernels' error word was raised. */
C_KZG_RET lwkzg_cell_group_device(uint32_t *rows, uint32_t *m_out, uint8_t *distinct48, uint32_t *first_item, uint32_t *perm_row,
                                  uint32_t *row_off, uint32_t *perm_col, uint32_t *col_off, uint32_t *bad_index,
                                  const void *commitments48_dev, const void *cell_indices_dev, size_t n, uint64_t seed, uint32_t hash_mask,
                                  void *stream);

/* PER-GROUP answers without a parked host thread: lwkzg_verify_cell_kzg_proof_groups_device (below) on a cell verifier (DESIGN.md
 * section 4r). The commitments and the indices never come to the host: the groups' de-duplication, rows, lists and slices are made by
 * kernels.
 *   lwkzg_cell_verifier_new_groups  everything lwkzg_cell_verifier_new allocates, plus what a grouped call of up to max_cells items in up
 *                                to max_groups groups needs (the segmented grouping's counters and lists, g power tables, the slice
 *                                table, 16 MiB for the interpolants, LWKZG_VERIFIER_DEPTH copies of the offsets), and the settings'
 *                                workspace for min(max_groups, 1024) MSM slots on both of the settings' contexts. The only call that
 *                                may allocate or synchronise the device. C_KZG_BADARGS also for max_groups == 0 or above 2^30. The
 *                                verifier takes lwkzg_cell_verifier_enqueue exactly as one from lwkzg_cell_verifier_new does; batch and
 *                                grouped calls may alternate, share its ring and its depth and complete in order; pending / wait /
 *                                free are unchanged, and free_trusted_setup waits for grouped calls in flight too. A verifier from
 *                                lwkzg_cell_verifier_new has max_groups == 0 and refuses a grouped call on the spot.
 *   lwkzg_cell_verifier_enqueue_groups  device item arrays (16-byte aligned, produced on `stream`; NULL = already complete) and HOST
 *                                group_offsets (g + 1 values, read -- copied into storage of the call's own job slot -- before the call
 *                                returns). For every j, (rc_out[j], ok_out[j]) is exactly what lwkzg_verify_cell_kzg_proof_groups_device
 *                                writes for the same inputs, in every mode and on both MSM engines: its definition, its precedence
 *                                inside a group, empty groups, and groups that do not spread to their neighbours. partials_out, if not
 *                                NULL, takes exactly what lwkzg_cell_verify_groups_partials writes. Nothing behind r runs on a bad
 *                                group's unvalidated points or unchecked indices. In *result:
 *                                    rc         the call's return code: C_KZG_OK once every group is decided
 *                                    ok         1 only if every group answered (C_KZG_OK, 1)
 *                                    first_bad  the lowest GROUP whose answer is anything else, 0xffffffff when there is none
 *                                    m          the total of the groups' distinct commitments
 *                                    partials   zero
 *                                ok_out, rc_out and partials_out (HOST arrays of g, g and g x LWKZG_CELL_VERIFY_PARTIAL_BYTES) are written
 *                                before result->state, which is stored last with release order: they stay the caller's -- not to be
 *                                read, reused or freed -- until it reads 1 there. The call returns once everything is enqueued: no wait
 *                                for a stream or an event, no allocation. Completed on the spot, as the call's return value:
 *                                C_KZG_BADARGS for group_offsets NULL, not starting at 0, not ending at n or not ascending, g == 0 with
 *                                n > 0, an item array NULL with n > 0, ok_out or rc_out NULL with g > 0, n above max_cells, g above
 *                                max_groups, a verifier from lwkzg_cell_verifier_new, and what lwkzg_cell_verifier_enqueue refuses
 *                                (nothing but *result is written); C_KZG_OK with ok = 1 for g == 0 with n == 0 (nothing else written)
 *                                and for n == 0 with g > 0 (every group is empty: (C_KZG_OK, 1) and zero partials for each, written
 *                                before the call returns). A failing enqueue: C_KZG_ERROR, as lwkzg_cell_verifier_enqueue. The stream
 *                                stands still while the host threads check the g pairings (about 0.4 ms per group and thread).
 * Not covered: host-pointer inputs, lwkzg_multi_* forms, stream capture, a pairing on the device. */
C_KZG_RET lwkzg_cell_verifier_new_groups(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_cells, size_t max_groups);
C_KZG_RET lwkzg_cell_verifier_enqueue_groups(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, uint8_t *ok_out /* HOST, g */,
                                             int32_t *rc_out /* HOST, g */,
                                             uint8_t *partials_out /* HOST, g x LWKZG_CELL_VERIFY_PARTIAL_BYTES, or NULL */,
                                             const void *commitments48_dev, const void *cell_indices_dev, const void *cells_dev,
                                             const void *proofs48_dev, size_t n, const uint64_t *group_offsets /* HOST, g + 1 */, size_t g,
                                             void *stream);
/* Test hook: lwkzg_cell_group_device for a call of g groups -- the segmented grouping kernels alone on device inputs and HOST offsets
 * (valid, n > 0, g > 0), every output brought to host arrays: rows n (GROUP-LOCAL; 0 for the items of a group with a bad index),
 * *m_out (M, the total of the groups' distinct commitments), distinct48 48 n (the groups' distinct commitments one after the other in
 * order of first occurrence, then infinity encodings), first_item n (M used), perm_row n / row_off n + 1 (M + 1 used) over the
 * concatenated rows, perm_col n / col_off 128 g + 1 (list 128 j + k), row_base g + 1, bad_words g (non-zero: an index of the group is
 * not below 128 -- it has no rows, columns or slices and its items are in no list). With slice_off_out (3 g + 1 words) and slices_out
 * (4 words -- group, sum, first, count -- for each of 3 (n / 64 + g) slices) not NULL the slice table too, cut with the groups flagged
 * by gflag (HOST, g words) or, where that is NULL, by the bad words. The order inside a list of perm_row / perm_col is not defined;
 * places of the two that no item took read 0xffffffff. seed, hash_mask, return codes: as lwkzg_cell_group_device. */
C_KZG_RET lwkzg_cell_group_segmented_device(uint32_t *rows, uint32_t *m_out, uint8_t *distinct48, uint32_t *first_item, uint32_t *perm_row,
                                            uint32_t *row_off, uint32_t *perm_col, uint32_t *col_off, uint32_t *row_base, uint32_t *bad_words,
                                            uint32_t *slices_out, uint32_t *slice_off_out, const uint32_t *gflag,
                                            const void *commitments48_dev, const void *cell_indices_dev, size_t n,
                                            const uint64_t *group_offsets /* HOST, g + 1 */, size_t g, uint64_t seed, uint32_t hash_mask,
                                            void *stream);
/* Host-only test hook: the two host steps of a grouped enqueue back to back on caller-supplied blocks, as
 * lwkzg_cell_verifier_host_steps; no GPU, no context. The blocks are what the device sends down for a call of n items in g groups:
 * group_offsets g + 1, row_base g + 1, bad_words g, status 2 n fault words ([i] item i's own, [n + q] concatenated row q's), first_item
 * (row_base[g] words), digests32 32 n, distinct48 (48 row_base[g] bytes), sums3x97 g x 3 x 97 and rli48 g x 48 (group j's at j). Per
 * group the answer into rc_out / ok_out and, where not NULL, partials_out; *out as lwkzg_cell_verifier_enqueue_groups completes it. A
 * rejected or empty group reads nothing behind what decides it: with a bad word set neither status nor digests, with a fault word set
 * neither digests nor sums; the blocks that only honest groups read may be NULL when there is none. */
C_KZG_RET lwkzg_cell_verifier_groups_host_steps(LwkzgCellVerifyResult *out, uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out,
                                                const uint64_t *group_offsets, size_t g, size_t n, const uint32_t *row_base,
                                                const uint32_t *bad_words, const int32_t *status, const uint32_t *first_item,
                                                const uint8_t *digests32, const uint8_t *distinct48, const uint8_t *sums3x97,
                                                const uint8_t *rli48, const KZGSettings *s, int mode);

/* Per-item cell verification: n independent lwkzg_verify_cell_kzg_proof_batch calls of ONE item each, in one. For every i, ok_out[i]
 * (0/1) and rc_out[i] (a C_KZG_RET) are exactly the (*ok, return code) of the batch call on item i alone, in the mode the settings
 * answer in; with one item the batch's r^0 = 1, so the check is e(C - [I(tau)]G1 + [c_k]pi, G2) e(-pi, g2_values[64]) == 1. A bad item
 * is an answer, not a failure:
 *     an index >= 128                                    rc C_KZG_BADARGS in both modes (decided first, whatever else is wrong), ok 0
 *     a commitment or a proof that is not a compressed
 *     point of G1 (infinity allowed), or a cell element
 *     not below r (never reduced)                        rc the mode's code (C_KZG_ERROR reference, C_KZG_BADARGS c-kzg), ok 0
 *     otherwise                                          rc C_KZG_OK, ok the verdict
 * and a good item's answer never depends on its neighbours. The call returns C_KZG_OK once every item is decided; C_KZG_BADARGS for
 * s NULL or any NULL pointer with n > 0; what the batch call refuses as a whole (no context, g2_values NULL) the same way;
 * C_KZG_MALLOC / C_KZG_ERROR only when the device work itself fails. n == 0: C_KZG_OK, nothing written. Synchronous. Every step runs on
 * the GPU, the pairing check of each item included. Verify a batch with lwkzg_verify_cell_kzg_proof_batch
 * first; this call is for a batch that answered false, or where every item needs its own answer. */
C_KZG_RET lwkzg_verify_cell_kzg_proof_each(uint8_t *ok_out, int32_t *rc_out, const Bytes48 *commitments, const uint64_t *cell_indices,
                                           const Cell *cells, const Bytes48 *proofs, size_t n, const KZGSettings *s);
/* the same for inputs already in HBM (device pointers, 16-byte aligned, produced on `stream`, NULL = already complete); the cells stay
 * on the device, the verdicts and codes come to the host */
C_KZG_RET lwkzg_verify_cell_kzg_proof_each_device(uint8_t *ok_out, int32_t *rc_out, const void *commitments48_dev,
                                                  const void *cell_indices_dev, const void *cells_dev, const void *proofs48_dev, size_t n,
                                                  const KZGSettings *s, void *stream);
/* test hook: the G1 point each item's pairing is taken of, by the verdict call's own code path up to the pairing. Per item
 * flag 1 | x 48 | y 48 big-endian: flag 0 = the affine point P_i = C_i - [I_i(tau)]G1 + [c_(k_i)]pi_i, 1 = P_i is the point at infinity
 * (rest zero), 2 = the item did not reach the combine (a bad item; rest zero). Host arguments and return codes as
 * lwkzg_verify_cell_kzg_proof_each. */
#define LWKZG_CELL_EACH_POINT_BYTES 97
C_KZG_RET lwkzg_cell_verify_each_points(uint8_t *out /* n x 97 */, const Bytes48 *commitments, const uint64_t *cell_indices,
                                        const Cell *cells, const Bytes48 *proofs, size_t n, const KZGSettings *s);

/* Per-group cell verification: g lwkzg_verify_cell_kzg_proof_batch calls in one, for a caller whose items come in units it must judge
 * one by one (the column sidecars of different peers, the blobs of different transactions). Group j is the items
 * group_offsets[j] .. group_offsets[j + 1] - 1 of the four item arrays (c-kzg-4844 2.x's item layout). For every j, rc_out[j] (a
 * C_KZG_RET) and ok_out[j] (0/1) are exactly the return code and *ok of the batch call on the items of group j alone, in the mode the
 * settings answer in and on every engine: the de-duplication and the row numbers, the transcript header's m and n, and r are the
 * group's own. Inside a group, as in the batch call:
 *     an index >= 128                                    rc C_KZG_BADARGS in both modes (decided first and on the host), ok 0
 *     a commitment or a proof that is not a compressed
 *     point of G1 (infinity allowed), or a cell element
 *     not below r                                        rc the mode's code (C_KZG_ERROR reference, C_KZG_BADARGS c-kzg), ok 0
 *     otherwise                                          rc C_KZG_OK, ok the verdict
 *     an empty group                                     rc C_KZG_OK, ok 1 (the batch call's answer to n == 0)
 * A bad group is an answer, not a failure, and does not spread: a good group's answer never depends on its neighbours, and nothing
 * behind r runs on a bad group's unvalidated points or unchecked indices. The call returns C_KZG_OK once every group is decided;
 * C_KZG_BADARGS, decided before any device work and with nothing written, for s NULL, ok_out / rc_out / group_offsets NULL with g > 0,
 * an item array NULL with n > 0, group_offsets[0] != 0, group_offsets[g] != n, offsets that do not ascend, and g == 0 with n > 0
 * (g == 0 with n == 0: C_KZG_OK, nothing written); what the batch call refuses as a whole (no context, g2_values NULL) the same way;
 * C_KZG_MALLOC / C_KZG_ERROR only when the device work itself fails. Synchronous. Per item the device does two scalar products and
 * some Fr work, per group one 64-term commitment; the pairing check of each group runs on the host threads.
 * Verify with lwkzg_verify_cell_kzg_proof_batch first; use this call when the answer must name the sidecar or the transaction, and
 * lwkzg_verify_cell_kzg_proof_each only for single cells.
 * The form that does not block is lwkzg_cell_verifier_enqueue_groups above.
 * Out of scope: lwkzg_multi_* forms, stream capture, and a pairing on the device (one lane's chain is about 90 ms; the host does a
 * group's check in about 0.40 ms per thread). */
C_KZG_RET lwkzg_verify_cell_kzg_proof_groups(uint8_t *ok_out, int32_t *rc_out, const Bytes48 *commitments, const uint64_t *cell_indices,
                                             const Cell *cells, const Bytes48 *proofs, size_t n,
                                             const uint64_t *group_offsets /* g + 1 */, size_t g, const KZGSettings *s);
/* the same for item arrays already in HBM (device pointers, 16-byte aligned, produced on `stream`, NULL = already complete). The
 * offsets stay a HOST array, read before the call returns. The commitments and the indices come down to be grouped; the cells never
 * leave the device. */
C_KZG_RET lwkzg_verify_cell_kzg_proof_groups_device(uint8_t *ok_out, int32_t *rc_out, const void *commitments48_dev,
                                                    const void *cell_indices_dev, const void *cells_dev, const void *proofs48_dev, size_t n,
                                                    const uint64_t *group_offsets /* HOST, g + 1 */, size_t g, const KZGSettings *s,
                                                    void *stream);
/* test hook: per group exactly what lwkzg_cell_verify_partials writes for the group alone (LWKZG_CELL_VERIFY_PARTIAL_BYTES each), by
 * the grouped call's own code path up to the pairings; all zero for an empty group and for a group whose rc is not C_KZG_OK. Host
 * arguments and return codes as lwkzg_verify_cell_kzg_proof_groups (out NULL with g > 0: C_KZG_BADARGS). */
C_KZG_RET lwkzg_cell_verify_groups_partials(uint8_t *out /* g x LWKZG_CELL_VERIFY_PARTIAL_BYTES */, const Bytes48 *commitments,
                                            const uint64_t *cell_indices, const Cell *cells, const Bytes48 *proofs, size_t n,
                                            const uint64_t *group_offsets /* g + 1 */, size_t g, const KZGSettings *s);

/* Cell proofs of WHOLE BLOBS: do the 128 cell proofs of each blob belong to the blob and its commitment? What the holder of a Fulu
 * blob transaction asks -- (blob, commitment, 128 proofs), no cells. Both calls are DEFINED by the calls above. For blob b let cells_b
 * be the 128 cells lwkzg_compute_cells_and_kzg_proofs(cells, NULL, &blobs[b], s) writes in the mode the settings answer in; the
 * expanded items of a call are the 128 n items (commitments[b], k, cells_b[k], cell_proofs[128 b + k]) in the order i = 128 b + k.
 *   batch    the return code and *ok are those of lwkzg_verify_cell_kzg_proof_batch on the expanded items: the same de-duplication
 *            of commitments, transcript and r. n == 0: C_KZG_OK, *ok = true.
 *   groups   group j is the BLOBS group_offsets[j] .. group_offsets[j + 1] - 1; rc_out[j] and ok_out[j] are those of
 *            lwkzg_verify_cell_kzg_proof_groups for the items 128 group_offsets[j] .. 128 group_offsets[j + 1] - 1 of the expanded
 *            items. An empty group answers (C_KZG_OK, 1); a bad group is an answer and does not spread.
 * A blob that the compute call rejects -- an element not below r in LWKZG_MODE_CKZG and LWKZG_MODE_ETH; reference mode reduces and
 * rejects nothing -- answers the mode's bad-input code, the code a cell element not below r gets: the batch call returns it with
 * *ok = false; in the groups call exactly the blob's own group takes it as rc_out[j] with ok_out[j] = 0, and nothing behind r runs on
 * that group. C_KZG_BADARGS, decided before any device work and with nothing written beyond *ok = false: s or ok NULL; blobs,
 * commitments or cell_proofs NULL with n > 0; for the groups call the list of lwkzg_verify_cell_kzg_proof_groups, with "item array"
 * read as these three and the offsets counting blobs. All three modes, every MSM engine; no proofs are computed, so the cell proof
 * engine (below) does not matter. Synchronous.
 * Memory: the cells live in a grow-only scratch of the settings object, 256 KiB + 16 bytes per blob (and, once, the host forms' upload
 * slice: 128 KiB per blob of the call, at most 8 MiB), beside what the call over 128 n items keeps; a second call of the same size
 * allocates nothing, free_trusted_setup frees it. C_KZG_MALLOC, the error text naming the size, when it does not fit.
 * Use these when you hold blobs; the calls over items when you hold cells.
 * The forms that do not block are lwkzg_cell_verifier_enqueue_blobs / _blobs_groups below.
 * Out of scope: lwkzg_multi_* forms, stream capture, versioned hashes, column sidecars in their own layout. */
C_KZG_RET lwkzg_verify_blob_cell_kzg_proofs_batch(bool *ok, const Blob *blobs, const Bytes48 *commitments /* n */,
                                                  const Bytes48 *cell_proofs /* n x 128 */, size_t n, const KZGSettings *s);
/* the same for inputs already in HBM (device pointers, 16-byte aligned, produced on `stream`, NULL = already complete). The blobs and
 * their cells never come to the host; the n commitments do, to be de-duplicated, and only n-entry tables go up. */
C_KZG_RET lwkzg_verify_blob_cell_kzg_proofs_batch_device(bool *ok, const void *blobs_dev, const void *commitments48_dev,
                                                         const void *cell_proofs48_dev, size_t n, const KZGSettings *s, void *stream);
/* test hook: exactly the bytes lwkzg_cell_verify_partials writes for the expanded items, by the verdict call's own code path */
C_KZG_RET lwkzg_blob_cell_verify_partials(uint8_t *out /* LWKZG_CELL_VERIFY_PARTIAL_BYTES */, const Blob *blobs, const Bytes48 *commitments,
                                          const Bytes48 *cell_proofs, size_t n, const KZGSettings *s);
C_KZG_RET lwkzg_verify_blob_cell_kzg_proofs_groups(uint8_t *ok_out, int32_t *rc_out, const Blob *blobs, const Bytes48 *commitments,
                                                   const Bytes48 *cell_proofs, size_t n,
                                                   const uint64_t *group_offsets /* in BLOBS, g + 1 */, size_t g, const KZGSettings *s);
/* device pointers as in the batch form; the offsets stay a HOST array, read before the call returns */
C_KZG_RET lwkzg_verify_blob_cell_kzg_proofs_groups_device(uint8_t *ok_out, int32_t *rc_out, const void *blobs_dev,
                                                          const void *commitments48_dev, const void *cell_proofs48_dev, size_t n,
                                                          const uint64_t *group_offsets /* HOST, in BLOBS, g + 1 */, size_t g,
                                                          const KZGSettings *s, void *stream);
/* test hook: per group exactly what lwkzg_cell_verify_groups_partials writes for the expanded items (out NULL with g > 0: C_KZG_BADARGS) */
C_KZG_RET lwkzg_blob_cell_verify_groups_partials(uint8_t *out /* g x LWKZG_CELL_VERIFY_PARTIAL_BYTES */, const Blob *blobs,
                                                 const Bytes48 *commitments, const Bytes48 *cell_proofs, size_t n,
                                                 const uint64_t *group_offsets /* in BLOBS, g + 1 */, size_t g, const KZGSettings *s);

/* Cell proofs of WHOLE BLOBS without a parked host thread: the two device forms above on a cell verifier.
 * Nothing of a call crosses to the host but what the verifier's two host functions read anyway: the blobs are extended into the
 * verifier's own scratch, the n commitments are de-duplicated by one workgroup on the device, and every list of the 128 n expanded
 * items is written there from its tables.
 *   lwkzg_cell_verifier_new_blobs  everything lwkzg_cell_verifier_new_groups(out, s, 128 max_blobs, max_groups) allocates (max_groups == 0:
 *                                what lwkzg_cell_verifier_new allocates), plus 256 KiB of cell scratch, 1 KiB of indices and 24 bytes of
 *                                tables and status per blob, and the settings' workspace for the extension of max_blobs blobs (two
 *                                slots per blob) on both of the settings' contexts. max_blobs is 1 .. 512 -- a call is one extension
 *                                chunk --, anything else C_KZG_BADARGS before any device work, as are the arguments
 *                                lwkzg_cell_verifier_new_groups refuses. The only one of these calls that may allocate or synchronise.
 *                                The verifier still takes lwkzg_cell_verifier_enqueue and, with max_groups > 0, _enqueue_groups;
 *                                calls of all four kinds share its ring and its depth and complete in order; pending / wait / free
 *                                are unchanged, and free_trusted_setup waits for blob calls in flight too. A verifier from
 *                                lwkzg_cell_verifier_new / _new_groups has no blob scratch and refuses a blob call on the spot.
 *   lwkzg_cell_verifier_enqueue_blobs  n device-resident blobs, n commitments and 128 n cell proofs (16-byte aligned, produced on
 *                                `stream`; NULL = already complete). *result gets what lwkzg_verify_blob_cell_kzg_proofs_batch_device
 *                                answers for the same inputs in the settings' mode and on every MSM engine: rc and ok; m, the number
 *                                of distinct commitments; partials, byte for byte what lwkzg_blob_cell_verify_partials writes (zero
 *                                unless rc == C_KZG_OK). first_bad counts EXPANDED ITEMS (i = 128 b + k): the lowest item whose own
 *                                cell, proof or commitment is at fault -- every item of a blob that the extension rejected counts
 *                                (128 b for the blob), and a bad commitment counts at 128 x the blob it was first seen at. A rejected
 *                                batch is an answer: the call returns C_KZG_OK and nothing behind r runs on it. n == 0 completes on
 *                                the spot with ok = 1. Completed on the spot as the return value: n above max_blobs, a NULL array
 *                                with n > 0, a freed setup, a verifier without blob scratch, and what lwkzg_cell_verifier_enqueue
 *                                refuses.
 *   lwkzg_cell_verifier_enqueue_blobs_groups  the same with HOST group_offsets counting BLOBS (g + 1 values, copied into the call's
 *                                job slot before the call returns). For every j, (rc_out[j], ok_out[j]) and the partials are exactly
 *                                those of lwkzg_verify_blob_cell_kzg_proofs_groups_device / lwkzg_blob_cell_verify_groups_partials;
 *                                *result as lwkzg_cell_verifier_enqueue_groups completes it (first_bad the lowest GROUP that is not
 *                                (C_KZG_OK, 1), m the total of the groups' distinct commitments). The completions on the spot are
 *                                those of lwkzg_cell_verifier_enqueue_groups with "item array" read as the three blob arrays, g == 0
 *                                with n == 0 and n == 0 with g > 0 included; a verifier made with max_groups == 0 refuses.
 * Both return once everything is enqueued: no wait for a stream or an event, no allocation, no copy of the commitments to the host.
 * Outputs are written before result->state, which is stored last with release order. Up to LWKZG_VERIFIER_DEPTH calls may be in
 * flight; one more waits for the oldest.
 * Not covered: host-pointer blobs, versioned hashes, column sidecars in their own layout, lwkzg_multi_* forms, stream capture, more
 * than one extension chunk per call, a pairing on the device. */
C_KZG_RET lwkzg_cell_verifier_new_blobs(LwkzgCellVerifier **out, const KZGSettings *s, size_t max_blobs, size_t max_groups);
C_KZG_RET lwkzg_cell_verifier_enqueue_blobs(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, const void *blobs_dev,
                                            const void *commitments48_dev, const void *cell_proofs48_dev, size_t n, void *stream);
C_KZG_RET lwkzg_cell_verifier_enqueue_blobs_groups(LwkzgCellVerifier *v, LwkzgCellVerifyResult *result, uint8_t *ok_out /* HOST, g */,
                                                   int32_t *rc_out /* HOST, g */,
                                                   uint8_t *partials_out /* HOST, g x LWKZG_CELL_VERIFY_PARTIAL_BYTES, or NULL */,
                                                   const void *blobs_dev, const void *commitments48_dev, const void *cell_proofs48_dev,
                                                   size_t n, const uint64_t *group_offsets /* HOST, in BLOBS, g + 1 */, size_t g,
                                                   void *stream);
/* Test hook, synchronous: the blob-level grouping and the expansion kernels alone, on n_blobs (1 .. 512) device-resident commitments
 * and HOST offsets in blobs (valid, g > 0). The outputs are those of lwkzg_cell_group_segmented_device for the 128 n_blobs expanded
 * items (n = 128 n_blobs in the sizes there; bad_words are zero; the slice table, where asked for, is cut with no group flagged), and,
 * where not NULL, item_group_out (n words) and cell_indices_out (n uint64). The order inside a list of perm_row / perm_col is not
 * defined. seed, hash_mask: of the keyed slot hash. C_KZG_BADARGS: NULL pointers, n_blobs 0 or above 512, bad offsets; C_KZG_ERROR:
 * the kernel's error word was raised. */
C_KZG_RET lwkzg_blob_group_device(uint32_t *rows, uint32_t *m_out, uint8_t *distinct48, uint32_t *first_item, uint32_t *perm_row,
                                  uint32_t *row_off, uint32_t *perm_col, uint32_t *col_off, uint32_t *row_base, uint32_t *bad_words,
                                  uint32_t *slices_out, uint32_t *slice_off_out, uint32_t *item_group_out, uint64_t *cell_indices_out,
                                  const void *commitments48_dev, size_t n_blobs, const uint64_t *group_offsets /* HOST, in BLOBS, g + 1 */,
                                  size_t g, uint64_t seed, uint32_t hash_mask, void *stream);

/* The engine behind the cell proofs of lwkzg_compute_cells_and_kzg_proofs* and lwkzg_recover_cells_and_kzg_proofs* (DESIGN.md section 4h),
 * a per-settings choice. FK20 (Feist-Khovratovich): the 128 proofs of a blob as a Toeplitz product over G1 -- 64 coefficient transforms,
 * 128 MSMs of 64 terms over a per-settings window table of 8192 transformed bases, and two 128-point transforms over G1 -- instead of 128
 * MSMs of 4096 terms. Same bytes, status words and return codes either way. The table: 8192 x 32 x 128 rows of 112 bytes, 3.5 GiB, at
 * the default width of 8 bits (widths 4, 6, 7, 8, 9 are supported); with the call's scratch it stays below the 8 GiB that the MSM tables
 * leave free. The transforms are a chain of thirteen dependent levels, so a call of few blobs is slower on FK20 than on the MSMs: */
#define LWKZG_CELL_PROOFS_MSM  0   /* 128 MSMs of 4096 terms per blob: DESIGN.md section 4h, the default */
#define LWKZG_CELL_PROOFS_FK20 1
#define LWKZG_FK20_DEFAULT_MIN_BLOBS 64   /* the smallest measured n from which FK20's median stays below the MSM path's: 64, from
                                          * profiles/fk20_timing.txt (tools/fk20_timing.py; 78.4 ms against 92.9 ms per call there, 87.1 against
                                          * 47.6 at n = 32); DESIGN.md section 4h */
/* engine FK20 builds the settings' FK20 table, then allocates everything an FK20 call needs. Calls allocate nothing afterwards.
 * window_bits 0 = the library's default width. min_blobs 0 = the library's default threshold.
 * A cell call (compute or recover) of fewer than min_blobs blobs keeps the MSM path.
 * engine MSM frees the table and the scratch.
 * C_KZG_MALLOC when the memory does not fit (or a transformed base is the point at infinity, which no real setup produces): the engine
 * stays unchanged and usable.
 * C_KZG_BADARGS for s NULL, an unknown engine or an unsupported width. Decided before any device work. */
C_KZG_RET lwkzg_set_cell_proof_engine(const KZGSettings *s, int engine, int window_bits, size_t min_blobs);
int    lwkzg_cell_proof_engine(const KZGSettings *s);   /* 0 / 1, -1 = bad settings */
size_t lwkzg_fk20_table_bytes(const KZGSettings *s);    /* 0 = no table */
size_t lwkzg_fk20_chunk_blobs(void);                    /* blobs per FK20 chunk: the tests cross it by one */
/* Test hook, run by the proof call's own code path, host pointers.
 * Per point: flag 1 (1 = infinity) | x 48 | y 48, big-endian, as lwkzg_cell_verify_partials writes them.
 *   what 0: the 8192 bases, Y^_i[m] at index 128 i + m (blob ignored)
 *   what 1: E[0..127] of the blob
 *   what 2: h_0 .. h_63 of the blob
 * C_KZG_ERROR when the settings' engine is not FK20. */
C_KZG_RET lwkzg_fk20_points(uint8_t *out, int what, const Blob *blob, const KZGSettings *s);

/* Host-only test hook for the per-item pairing: the 68 lines of the Miller loop of a ZCash-compressed G2 point (not at infinity) as the
 * device takes them, canonical big-endian lambda.c0 | lambda.c1 | c0.c0 | c0.c1 per line (out: 68 x 192 bytes). No GPU, no settings. */
C_KZG_RET lwkzg_pairing_line_table(uint8_t *out, const uint8_t *g2_compressed);

/* Host-only test hook for the verify side: prod_i e(P_i, Q_i) == 1 for up to 4 pairs of ZCash-compressed
 * points (G1 48 bytes, G2 96 bytes; a pair with a point at infinity contributes 1). No GPU, no settings. */
C_KZG_RET lwkzg_pairing_product_is_one(bool *ok, const uint8_t *g1_compressed, const uint8_t *g2_compressed, size_t n);

/* Host-only test hook: digests[i] = SHA-256("FSBLOBVERIFY_V1_" | le64(4096) | le64(0) | blobs[i] | commitments[i]),
 * the compute_challenge message (src/utils.rs:120-144), as the host-pointer proof entry points compute it. */
C_KZG_RET lwkzg_challenge_digests_host(uint8_t *digests32, const uint8_t *blobs, const uint8_t *commitments48, size_t n);
/* the same for `mode`'s message: modes 0 and 1 hash what the hook above hashes, LWKZG_MODE_ETH hashes
 * "FSBLOBVERIFY_V1_" | be128(4096) | blobs[i] | commitments[i]. C_KZG_BADARGS for an unknown mode. */
C_KZG_RET lwkzg_challenge_digests_host_mode(uint8_t *digests32, const uint8_t *blobs, const uint8_t *commitments48, size_t n, int mode);

/* Host-only: the batch challenge of verify_blob_kzg_proof_batch (src/utils.rs:166-206) over a transcript of n_total 160-byte records
 * (lwkzg_verify_shard_begin*'s output, all shards in order): r = SHA-256("RCKZGBATCH___V1_" | le64(4096) | le64(n_total) | records) read as a
 * field element in `mode`'s byte order and reduced (LWKZG_MODE_ETH: the header's two fields are be64); r_out = its canonical value, 32 bytes big-endian. What every shard derives inside
 * lwkzg_verify_shard_partial; exposed so that a sharded verifier can log / cross-check it (tests hold it against hashlib). */
C_KZG_RET lwkzg_batch_challenge_host(uint8_t r_out[32], const uint8_t *records_all, size_t n_total, int mode);

/* Engine introspection / profiling (bench.py). With the profile on, a kernel's time is read from a hipEvent pair bound to its own
 * dispatch (no packet beside the launch); scopes of more than one launch are timed by two marker packets on the launch stream. */
int lwkzg_device_count(void);
int lwkzg_set_device(int ordinal);                 /* device used by subsequent load_* calls */
const char *lwkzg_version(void);
const char *lwkzg_last_error(void);                /* thread-local, human readable */
void lwkzg_profile_enable(int on);
void lwkzg_profile_reset(void);
/* JSON: {"kernel": {"launches": n, "total_ms": t}, ...}; returns bytes needed (incl. NUL) */
size_t lwkzg_profile_report(char *buf, size_t cap);
/* Test hook. JSON: what the profile has been made of since the last lwkzg_profile_reset -- {"dispatch_pairs": pairs bound to a launch's
 * own dispatch, "marker_pairs": scopes timed by marker packets, "shared_markers": of those, scopes whose opening marker is the closing
 * marker of the scope in front, "event_flags": the hipEventCreateWithFlags flags of the pooled event created last}; returns bytes needed
 * (incl. NUL). tests/test_gpu_dispatch_events.py reads it. */
size_t lwkzg_profile_sources(char *buf, size_t cap);
/* JSON: the wall-clock milliseconds of this settings object's load (context, points + tables, G2 + FFT settings, the
 * default engine's table) and of its last lwkzg_enable_direct_table: freeing the old table, the hipMallocs of the new one
 * (one per window, summed: the GPU builds window j while the host allocates window j + 1), scratch, and what was left of the
 * build kernels after the last allocation returned; returns bytes needed (incl. NUL). The allocations return in a millisecond on idle memory
 * and wait ~25 ms per GB for the driver's scrub of memory released shortly before (tools/alloc_pieces.hip). */
size_t lwkzg_timing_report(const KZGSettings *s, char *buf, size_t cap);
/* JSON: the environment knobs in effect for this process -- read ONCE, in one place (csrc/knobs.h). "operational" and "experimental"
 * list the variable names; experiment knobs (A/B arms of measurements) are honoured only with LWKZG_EXPERIMENTAL=1 and are otherwise
 * ignored (reported under LWKZG_VERBOSE). Returns bytes needed (incl. NUL). INTEGRATION.md section 5 documents the operational ones. */
size_t lwkzg_knob_report(char *buf, size_t cap);
/* Test hook: the schedule (csrc/plan.h: ProofSchedule, 0 = small-host .. 4 = GPU chains) the most recent
 * lwkzg_compute_blob_kzg_proof_batch_device call of this process took, -1 before the first. tests/test_gpu_plan.py forces each schedule
 * once (LWKZG_EXPERIMENTAL=1 LWKZG_PROOF_SCHEDULE=k) and reads it back. */
int lwkzg_last_proof_schedule(void);

/* First use of the HIP runtime by this process (device context + this library's code object), so that a caller can pay
 * and time it apart from its first real call. 0, or -1 without a GPU. */
int lwkzg_runtime_init(void);
/* The shader clock (MHz) the current device holds under ~0.4 ms of dense multiply-adds on every SIMD (clock64 against the 100 MHz
 * wall clock). A measurement aid: bench.py prints it with a hash of the GPU's uuid so that profiles can be matched to boxes. */
C_KZG_RET lwkzg_clock_probe_mhz(double *mhz);
/* MSM plan constants, for roofline arithmetic in bench.py */
int lwkzg_msm_window_bits(void);
int lwkzg_msm_num_windows(void);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* LAMBDAWORKS_KZG_AMD_H */
