// validate.hip -- G1 point validation on the GPU: what every verifying entry point does to its commitments and proofs first (blob
// proofs, batch and per-item verification, the cell verifiers, the sharded form). One kernel for the whole chain (k_validate_commitments,
// r04's arm), or square root (k_decompress_points) | subgroup test on a quad of lanes (k_subgroup_coop_asm) | canonical bytes and
// verdicts (k_subgroup_canon), over one point set or two per launch. The launches that carry an LDS footprint go through lds_pad.h.
#include "kernels.h"
#include "knobs.h"
#include "lds_pad.h"

namespace lwk {

// decompress_g1_point (incl. the subgroup check) then compress_g1_point again, as compute_blob_kzg_proof +
// compute_challenge do (/root/reference/src/lib.rs:372-375, src/utils.rs:138). One lane per point, all in the
// lazy-limb field (field29.cuh): square root (p = 3 mod 4), root selection by the sign flag, endomorphism subgroup
// test. Re-compressing an affine point needs no inversion: the canonical bytes are x (reduced) + flags.
// aff_out / kind_out (optional): the validated point in the hot-loop representation and 0 = affine,
// 1 = infinity, 2 = invalid, for the verify side's linear combinations.
__global__ __launch_bounds__(64) void k_validate_commitments(const uint8_t *__restrict__ comm48,
                                                             uint8_t *__restrict__ canon48, int32_t *__restrict__ status,
                                                             int bad_code, size_t n, G1Affine29 *__restrict__ aff_out,
                                                             int32_t *__restrict__ kind_out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    __builtin_amdgcn_s_setprio(2);  // a latency chain, like the hash kernel it runs beside (see there)
    G1Affine29 aff;
    aff.x = F29<2>::zero();
    aff.y = F29<2>::zero();
    uint8_t o[48];
    for (int k = 0; k < 48; k++) o[k] = 0;
    F29<2> x = F29<2>::zero(), y = F29<2>::zero();
    bool want_greater = false;
    int rc = g1_decompress29_nocheck(comm48 + 48 * i, x, y, want_greater);
    if (rc == 1) {
        o[0] = 0xc0;
    } else if (rc == 0) {
        uint32_t braw[12];
        g1_beta_raw(braw);
        if (!g1_in_subgroup_endo<G1Xyzz29>(x, y, f29_from_raw32(braw))) {
            rc = 2;
        } else {
            uint32_t rx[12];
            f29_to_raw32(rx, x);
            raw_to_be<12>(o, rx);
            o[0] |= 0x80;
            if (want_greater) o[0] |= 0x20;
            aff.x = x;
            aff.y = y;
        }
    }
    if (rc == 2) {
        status[i] = bad_code;
        for (int k = 0; k < 48; k++) o[k] = 0;
    }
    for (int k = 0; k < 48; k++) canon48[48 * i + k] = o[k];
    if (aff_out) aff_out[i] = aff;
    if (kind_out) kind_out[i] = rc;
}

void launch_validate_commitments(const uint8_t *comm48, uint8_t *canon48, int32_t *status, int bad_code, size_t n,
                                 hipStream_t st, G1Affine29 *aff_out, int32_t *kind_out, uint32_t *verdict_scratch, bool apart) {
    // r05: with scratch for the points and the verdicts the validation is three launches -- the square root (one lane per point, windowed),
    // the subgroup test on a quad of lanes per point (k_subgroup_coop_asm), canonical bytes + verdicts -- 2.0 -> ~1.0 ms whatever the batch
    if (aff_out && kind_out && verdict_scratch && n && knobs().validate_coop) {
        const PointSet set{comm48, aff_out, kind_out, canon48, verdict_scratch};
        launch_decompress_points(set, nullptr, n, st, apart);
        launch_subgroup_canon(set, nullptr, status, bad_code, n, st, apart, true);
        return;
    }
    ProfScope p("k_validate_commitments", st);
    // The kernel is a one-wave-per-workgroup latency chain that runs beside other latency chains (the Fiat-Shamir hash of the device-resident
    // proofs, the other point set's validation). Where a wave of each shares a SIMD, both run at about half speed, and the dispatcher likes to
    // start every kernel's workgroups on the same compute units. An LDS footprint the kernel never touches keeps them apart: 112 KB here + the
    // hash kernel's 48 KB (or a second validation workgroup) exceed the 160 KB of a compute unit. The hash of 1024 blobs takes 3.2 ms instead
    // of 4.3 ms beside it (LWKZG_VALIDATE_LDS_PAD=0 switches the padding off).
    static PadCache cache;
    launch_padded(cache, (const void *)k_validate_commitments, knobs().validate_lds_pad, [&](unsigned lds) {
        hipLaunchKernelGGL(k_validate_commitments, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, st, comm48, canon48, status, bad_code, n,
                           aff_out, kind_out);
    });
}

// ---- the same validation in two launches, for the batch verification ------------------------------------------------
// k_decompress_points: square root only. k_subgroup_canon: subgroup test + canonical bytes + verdicts. What lies
// between them is the point of the split: the multiples the linear combinations want (setup.hip: k_point_multiples) need
// the decompressed point but not the subgroup verdict, so they run BESIDE the second kernel instead of behind it.
// kind carries the sign bit in bit 8 between the two kernels (rc | want_greater << 8) and is final (0 / 1 / 2) after
// the second; readers in between mask with 0xff.

// The square root's chain for a lane that is alone on its SIMD (256 commitments are four waves): f29_pow's 4-bit windows with the products
// INLINED (a call costs the lone wave ~40 instruction slots of moves, 475 times) and the 16-entry window table in LDS, [entry][limb][lane]
// (the exponent is public: every lane reads the same entry, its own column; the table indexed by a run-time digit would otherwise live
// in scratch, a memory round trip per window).
__device__ __forceinline__ F29<2> sqrt_chain_lds(const F29<2> &a, const uint32_t *e, uint32_t (*tab)[14][64], int lane) {
    typedef F29<2, true> Fi;
    Fi t1;
#pragma unroll
    for (int j = 0; j < 14; j++) t1.l[j] = a.l[j];
    t1 = t1 * F29<1, true>::one();
    const Fi one = Fi::one();
#pragma unroll
    for (int j = 0; j < 14; j++) {
        tab[0][j][lane] = one.l[j];
        tab[1][j][lane] = t1.l[j];
    }
    Fi cur = t1;
#pragma unroll 1
    for (int k = 2; k < 16; k++) {
        cur = cur * t1;
#pragma unroll
        for (int j = 0; j < 14; j++) tab[k][j][lane] = cur.l[j];
    }
    Fi acc = one;
    bool started = false;
#pragma unroll 1
    for (int w = 12 * 8 - 1; w >= 0; w--) {
        const uint32_t d = (e[w >> 3] >> (4 * (w & 7))) & 15u;
        if (started) {
            acc = sqr(acc);
            acc = sqr(acc);
            acc = sqr(acc);
            acc = sqr(acc);
        }
        if (d) {
            Fi f;
#pragma unroll
            for (int j = 0; j < 14; j++) f.l[j] = tab[d][j][lane];
            acc = started ? acc * f : f;
            started = true;
        }
    }
    F29<2> r;
#pragma unroll
    for (int j = 0; j < 14; j++) r.l[j] = acc.l[j];
    return r;
}

// blockIdx.y selects one of two point sets (a verification's proofs and commitments in one launch; a single set passes itself twice)
__global__ __launch_bounds__(64) void k_decompress_points(const uint8_t *__restrict__ in48_a, G1Affine29 *__restrict__ pts_a,
                                                          int32_t *__restrict__ kind_a, const uint8_t *__restrict__ in48_b,
                                                          G1Affine29 *__restrict__ pts_b, int32_t *__restrict__ kind_b, size_t n) {
    __shared__ uint32_t tab[16][14][64];   // 56 KiB: two workgroups to a compute unit
    const uint8_t *in48 = blockIdx.y ? in48_b : in48_a;
    G1Affine29 *pts = blockIdx.y ? pts_b : pts_a;
    int32_t *kind = blockIdx.y ? kind_b : kind_a;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F29<2> x = F29<2>::zero(), y = F29<2>::zero();
    bool want_greater = false;
    const int lane = threadIdx.x;
    const int rc = g1_decompress29_nocheck_t(in48 + 48 * i, x, y, want_greater,
                                             [&](const F29<2> &a, const uint32_t *e) { return sqrt_chain_lds(a, e, tab, lane); });
    G1Affine29 aff;
    aff.x = rc == 0 ? x : F29<2>::zero();
    aff.y = rc == 0 ? y : F29<2>::zero();
    pts[i] = aff;
    kind[i] = rc | (want_greater ? 0x100 : 0);
}

// verdict (optional): the cooperative subgroup test's word per point (k_subgroup_coop_asm: 0 = not in G1, 1 = in G1, 2 = undetermined --
// an addition met P = +-Q in its low 56 bits --, which this kernel settles with the complete-branches test)
__global__ __launch_bounds__(64) void k_subgroup_canon(G1Affine29 *__restrict__ pts_a, int32_t *__restrict__ kind_a,
                                                       uint8_t *__restrict__ canon48_a, const uint32_t *__restrict__ verdict_a,
                                                       G1Affine29 *__restrict__ pts_b, int32_t *__restrict__ kind_b,
                                                       uint8_t *__restrict__ canon48_b, const uint32_t *__restrict__ verdict_b,
                                                       int32_t *__restrict__ status, int bad_code, size_t n) {
    G1Affine29 *pts = blockIdx.y ? pts_b : pts_a;
    int32_t *kind = blockIdx.y ? kind_b : kind_a;
    uint8_t *canon48 = blockIdx.y ? canon48_b : canon48_a;
    const uint32_t *verdict = blockIdx.y ? verdict_b : verdict_a;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k0 = kind[i];
    int rc = k0 & 0xff;
    uint8_t o[48];
    for (int k = 0; k < 48; k++) o[k] = 0;
    if (rc == 1) {
        o[0] = 0xc0;
    } else if (rc == 0) {
        const G1Affine29 aff = pts[i];
        const uint32_t vd = verdict ? verdict[i] : 2u;
        bool in_g1 = vd == 1u;
        if (vd >= 2u) {
            uint32_t braw[12];
            g1_beta_raw(braw);
            in_g1 = g1_in_subgroup_endo<G1Xyzz29>(aff.x, aff.y, f29_from_raw32(braw));
        }
        if (!in_g1) {
            rc = 2;
            G1Affine29 z;
            z.x = F29<2>::zero();
            z.y = F29<2>::zero();
            pts[i] = z;
        } else {
            uint32_t rx[12];
            f29_to_raw32(rx, aff.x);
            raw_to_be<12>(o, rx);
            o[0] |= 0x80;
            if (k0 & 0x100) o[0] |= 0x20;
        }
    }
    if (rc == 2) status[i] = bad_code;
    for (int k = 0; k < 48; k++) canon48[48 * i + k] = o[k];
    kind[i] = rc;
}

void launch_decompress_points(const PointSet &a, const PointSet *b2, size_t n, hipStream_t st, bool apart) {
    const PointSet &b = b2 ? *b2 : a;
    ProfScope p("k_decompress_points", st, kProfHandsOver);
    static PadCache cache;
    launch_padded(cache, (const void *)k_decompress_points, apart ? knobs().verify_pad_kb[0] * 1024u : 0u, [&](unsigned lds) {
        hipLaunchKernelGGL(k_decompress_points, dim3((unsigned)((n + 63) / 64), b2 ? 2 : 1), dim3(64), lds, st, a.in48, a.pts, a.kind, b.in48,
                           b.pts, b.kind, n);
    });
}

// The subgroup test on a QUAD of lanes per point (tools/gen_subgroup_asm.py writes subgroup_asm.inc and explains it): doublings in three
// rounds of one product per lane, the cooperative MSM kernel's addition, the public bits of |z| as a scalar loop. Workgroups of four
// unrelated waves (one per SIMD of a compute unit), 16 points per wave.
__global__ __launch_bounds__(256) void k_subgroup_coop_asm(const G1Affine29 *__restrict__ pts_a, const int32_t *__restrict__ kind_a,
                                                           uint32_t *__restrict__ verdict_a, const G1Affine29 *__restrict__ pts_b,
                                                           const int32_t *__restrict__ kind_b, uint32_t *__restrict__ verdict_b, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const G1Affine29 *pts = blockIdx.y ? pts_b : pts_a;
    const int32_t *kind = blockIdx.y ? kind_b : kind_a;
    uint32_t *verdict = blockIdx.y ? verdict_b : verdict_a;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t first = (blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * 16;
    __builtin_amdgcn_s_setprio(2);
    asm volatile(
#include "subgroup_asm.inc"
        :
        : "s"(pts), "s"(kind), "s"(verdict), "s"(n), "s"(first), "v"(lane)
        :
#include "subgroup_asm_clobbers.inc"
    );
#endif
}

// the quad test (two sets: always, as r06 shipped it; one set: with verdict scratch and validate_coop on), then canonical bytes and verdicts
void launch_subgroup_canon(const PointSet &a, const PointSet *b2, int32_t *status, int bad_code, size_t n, hipStream_t st, bool apart,
                           bool behind_decompress) {
    const PointSet &b = b2 ? *b2 : a;
    const dim3 grid((unsigned)((n + 63) / 64), b2 ? 2 : 1);
    const bool coop = b2 || (a.verdict && knobs().validate_coop);
    if (coop) {
        ProfScope p("k_subgroup_coop_asm", st, behind_decompress ? kProfTakesOver : 0u);
        static PadCache cache;
        launch_padded(cache, (const void *)k_subgroup_coop_asm, apart ? knobs().verify_pad_kb[1] * 1024u : 0u, [&](unsigned lds) {
            hipLaunchKernelGGL(k_subgroup_coop_asm, grid, dim3(256), lds, st, a.pts, a.kind, a.verdict, b.pts, b.kind, b.verdict, (uint32_t)n);
        });
    }
    prof_launch("k_subgroup_canon", st, k_subgroup_canon, grid, dim3(64), 0, a.pts, a.kind, a.canon48, coop ? a.verdict : nullptr, b.pts, b.kind,
                b.canon48, coop ? b.verdict : nullptr, status, bad_code, n);
}

}  // namespace lwk
