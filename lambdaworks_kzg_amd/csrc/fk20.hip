// fk20.hip -- the kernels of the FK20 cell proof engine (the pipeline and the table's life are fk20_api.hip).
//
// The 128 cell proofs of a blob are F[rev7(k)], F the forward 128-point transform over G1 of (h_0 .. h_63, O x 64), and the h_u are a
// Toeplitz product of the blob's coefficients with the setup. Per blob:
//   k_fk20_coeffs      64 Fr transforms of 128 points, one wave each: A^_i of the gathered coefficients, written as MSM scalars [m][i]
//   k_fk20_msm         128 MSMs of 64 terms over the window table of the transformed bases Y^_i[m], one wave each: E[m]
//   k_fk20_transforms  one workgroup of 128 lanes: the inverse transform of E (first 64 outputs, scaled by 1/128: h_u), then the
//                      forward transform of (h, O x 64); a level is one fixed-root product per lane and one complete addition
// and the existing k_finalize_compress behind them. The table side: k_fk20_base_rows (the scalar rows whose commitments are the bases)
// and k_fk20_table (all multiples of every base, per window).
#include "fk20.cuh"
#include "kernels.h"

namespace lwk {

// ---- table build ---------------------------------------------------------------------------------------------------------------------

// Row b = 128 i + m of a launch set (rows first .. first + n_rows): the 4096 scalars whose commitment over the monomial setup is
// Y^_i[m] = sum_{j <= 62} w^(m j) G[64 (62 - j) + i]. roots_raw: w^e, e < 128, canonical limbs. One lane per scalar.
__global__ __launch_bounds__(256) void k_fk20_base_rows(uint4 *__restrict__ rows, const uint4 *__restrict__ roots_raw, uint32_t first,
                                                        size_t n) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint32_t b = first + (uint32_t)(g / kBlobElems), t = (uint32_t)(g % kBlobElems);
    const uint32_t i = b / kFk20Points, m = b % kFk20Points;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if ((t % kFk20Terms) == i && t / kFk20Terms <= 62) {
        const uint32_t j = 62 - t / kFk20Terms, e = (m * j) % kFk20Points;
        lo = roots_raw[2 * e];
        hi = roots_raw[2 * e + 1];
    }
    rows[2 * g] = lo;
    rows[2 * g + 1] = hi;
}

void launch_fk20_base_rows(uint32_t *rows_raw, const uint32_t *roots_raw, uint32_t first, size_t n_rows, hipStream_t st) {
    const size_t n = n_rows * kBlobElems;
    prof_launch("k_fk20_base_rows", st, k_fk20_base_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (uint4 *)rows_raw, (const uint4 *)roots_raw,
                first, n);
}

// One lane per (base, window): Q = [2^(c j)]B by doublings, then rows d = 1 .. h as Q, 2Q, .. by mixed additions, each brought to
// affine form with an inversion of its own (46 ms per settings object at the default width: it does not ask for more). bases: index
// 128 i + m, none at infinity (fk20_api.hip refuses such a setup before this runs).
__global__ __launch_bounds__(256) void k_fk20_table(const G1Affine *__restrict__ bases, G1Affine29 *__restrict__ table, Fk20Plan plan) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)kFk20Bases * plan.nw) return;
    const uint32_t b = (uint32_t)(g / plan.nw), j = (uint32_t)(g % plan.nw);
    G1Affine29 q = affine_to_29(bases[b]);
    if (j) {
        G1Xyzz29 cur = G1Xyzz29::from_affine(q.x, q.y);
        for (uint32_t d = 0; d < j * (uint32_t)plan.c; d++) cur = xyzz_dbl(cur);
        q = xyzz29_to_affine29(cur);   // never infinity: B has prime order r
    }
    G1Affine29 *rows = table + fk20_row(plan, b / kFk20Points, b % kFk20Points, j, 1);
    rows[0] = q;
    G1Xyzz29 cur = G1Xyzz29::from_affine(q.x, q.y);
    for (uint32_t d = 1; d < plan.h; d++) {
        cur = xyzz_madd(cur, q.x, q.y);
        rows[d] = xyzz29_to_affine29(cur);
    }
}

void launch_fk20_table(const G1Affine *bases, G1Affine29 *table, int bits, hipStream_t st) {
    const Fk20Plan plan = fk20_plan(bits);
    const size_t n = (size_t)kFk20Bases * plan.nw;
    prof_launch("k_fk20_table", st, k_fk20_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, bases, table, plan);
}

// ---- coefficient transforms ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ Fr fk20_load_raw(const uint4 *p, size_t i) {
    const uint4 lo = p[2 * i], hi = p[2 * i + 1];
    Fr v;
    v.l[0] = lo.x, v.l[1] = lo.y, v.l[2] = lo.z, v.l[3] = lo.w;
    v.l[4] = hi.x, v.l[5] = hi.y, v.l[6] = hi.z, v.l[7] = hi.w;
    return v;
}

constexpr int kCoeffWaves = 4;   // (blob, i) pairs per workgroup: i = 4 blockIdx.x % 64 .., so that a workgroup writes 128 contiguous bytes per m

// One wave per (blob, i): A_i[0] = p[4032 + i], A_i[m] = 0 for 1 <= m <= 65, A_i[m] = p[64 (m - 65) + i] beyond, gathered into LDS in
// bit-reversed positions; seven decimation-in-time levels, a butterfly per lane, on the raw canonical values (the product of a raw
// value with a Montgomery-form twiddle is the raw product); out[blob][m][i] canonical limbs: one MSM's 64 scalars are contiguous.
__global__ __launch_bounds__(64 * kCoeffWaves) void k_fk20_coeffs(const uint4 *__restrict__ coeffs_raw, const Fr *__restrict__ tw_fwd,
                                                                  uint4 *__restrict__ out) {
    __shared__ Fr buf[kCoeffWaves][kFk20Points];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t pair = (size_t)blockIdx.x * kCoeffWaves + wave;
    const size_t blob = pair / kFk20Terms;
    const uint32_t i = (uint32_t)(pair % kFk20Terms);
    const uint4 *p = coeffs_raw + blob * kBlobElems * 2;
    Fr *x = buf[wave];
#pragma unroll
    for (uint32_t half = 0; half < 2; half++) {
        const uint32_t pos = lane + 64 * half, m = __brev(pos) >> 25;
        Fr v = Fr::zero();
        if (m == 0) v = fk20_load_raw(p, kBlobElems - kFk20Terms + i);
        else if (m >= 66) v = fk20_load_raw(p, (size_t)kFk20Terms * (m - 65) + i);
        x[pos] = v;
    }
    __syncthreads();
    for (uint32_t h = 1; h < (uint32_t)kFk20Points; h <<= 1) {
        const uint32_t k = lane & (h - 1), lo = ((lane & ~(h - 1)) << 1) | k;
        const Fr u = x[lo];
        const Fr t = tw_fwd[32 * k * (kFk20Points / 2 / h)] * x[lo + h];   // w128^e = w4096^(32 e), e < 64
        x[lo] = u + t;
        x[lo + h] = u - t;
        __syncthreads();
    }
#pragma unroll
    for (uint32_t half = 0; half < 2; half++) {
        const uint32_t m = lane + 64 * half;
        const Fr v = x[m];
        const size_t o = ((blob * kFk20Points + m) * kFk20Terms + i) * 2;
        out[o] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
        out[o + 1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
    }
}

void launch_fk20_coeffs(const uint32_t *coeffs_raw, const Fr *tw_fwd, uint32_t *scalars_out, size_t n_blobs, hipStream_t st) {
    prof_launch("k_fk20_coeffs", st, k_fk20_coeffs, dim3((unsigned)(n_blobs * kFk20Terms / kCoeffWaves)), dim3(64 * kCoeffWaves), 0,
                (const uint4 *)coeffs_raw, tw_fwd, (uint4 *)scalars_out);
}

// ---- the 64-term MSMs ----------------------------------------------------------------------------------------------------------------

// One wave per (m, blob), the grid m-major so that the blobs in flight share table rows in L2; lane i owns term i: its scalar's signed
// digits pick one row per window, summed by mixed additions; the 64 lane sums fold in a six-level tree of complete additions through
// LDS. E[m] goes to position rev7(m) of the blob's 128 points: the order the inverse transform reads.
__global__ __launch_bounds__(64) void k_fk20_msm(const G1Affine29 *__restrict__ table, Fk20Plan plan, const uint4 *__restrict__ scalars,
                                                 G1Xyzz29 *__restrict__ e_out, uint32_t n_blobs) {
    __shared__ G1Xyzz29 sh[kFk20Terms];
    const uint32_t t = threadIdx.x;
    const uint32_t m = blockIdx.x / n_blobs, blob = blockIdx.x % n_blobs;
    const size_t s = ((size_t)blob * kFk20Points + m) * kFk20Terms + t;
    const uint4 lo = scalars[2 * s], hi = scalars[2 * s + 1];
    uint32_t k[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const G1Affine29 *rows = table + fk20_row(plan, t, m, 0, 1);
    G1Xyzz29 acc = G1Xyzz29::infinity();
    uint32_t carry = 0;
#pragma unroll 1
    for (int j = 0; j < plan.nw; j++) {
        uint32_t mag, negative;
        fk20_next_digit(k, plan.c, j == plan.nw - 1, carry, mag, negative);
        if (mag > plan.h) mag = plan.h;   // (only the scalars of a blob whose status word rejects it can be out of range: stay inside the table)
        if (mag) {
            const G1Affine29 row = rows[(size_t)j * plan.h + (mag - 1)];
            acc = xyzz_madd(acc, row.x, cneg(row.y, negative != 0));
        }
    }
    for (uint32_t d = 1; d < (uint32_t)kFk20Terms; d <<= 1) {
        if ((t & (2 * d - 1)) == d) sh[t] = acc;
        __syncthreads();
        if ((t & (2 * d - 1)) == 0) acc = xyzz_add(acc, sh[t + d]);
        __syncthreads();
    }
    if (t == 0) e_out[(size_t)blob * kFk20Points + (__brev(m) >> 25)] = acc;
}

void launch_fk20_msm(const G1Affine29 *table, int bits, const uint32_t *scalars, G1Xyzz29 *e_out, size_t n_blobs, hipStream_t st) {
    prof_launch("k_fk20_msm", st, k_fk20_msm, dim3((unsigned)(n_blobs * kFk20Points)), dim3(64), 0, table, fk20_plan(bits), (const uint4 *)scalars,
                e_out, (uint32_t)n_blobs);
}

// ---- the two G1 transforms -----------------------------------------------------------------------------------------------------------

// One workgroup per blob, one lane per position, the 128 points in LDS (28 KiB). pts: E in bit-reversed positions in, the 128 proof
// points (position k = proof k) out. roots: kFk20Roots recoded roots of kFk20RootDigits bytes (fk20.cuh). h_out: when given, h_0 .. h_63
// of every blob are left there as well (the test hook). Every level is "take your root" and "take your sum or difference", a barrier
// between the two and around the stores: thirteen levels, twelve of them with a 130-doubling product in front.
__global__ __launch_bounds__(kFk20Points) void k_fk20_transforms(G1Xyzz29 *__restrict__ pts, const uint8_t *__restrict__ roots, F29<2> beta,
                                                                 G1Xyzz29 *__restrict__ h_out) {
    __shared__ G1Xyzz29 x[kFk20Points];
    const uint32_t pos = threadIdx.x;
    G1Xyzz29 *mine = pts + (size_t)blockIdx.x * kFk20Points;
    x[pos] = mine[pos];
    __syncthreads();
#pragma unroll 1
    for (uint32_t h = 1; h < (uint32_t)kFk20Points; h <<= 1) {
        const int root = fk20_inverse_root(pos, h);
        if (root) x[pos] = fk20_mul_root(x[pos], roots + (size_t)root * kFk20RootDigits, beta);   // (a lane touches its own point only)
        __syncthreads();
        const G1Xyzz29 out = fk20_inverse_out(x, pos, h);
        __syncthreads();
        x[pos] = out;
        __syncthreads();
    }
    if (h_out && pos < (uint32_t)kFk20Terms) h_out[(size_t)blockIdx.x * kFk20Terms + pos] = x[pos];
#pragma unroll 1
    for (uint32_t h = kFk20Points / 2; h >= 1; h >>= 1) {
        G1Xyzz29 out = fk20_forward_out(x, pos, h);
        const int root = fk20_forward_root(pos, h);
        if (root) out = fk20_mul_root(out, roots + (size_t)root * kFk20RootDigits, beta);
        __syncthreads();
        x[pos] = out;
        __syncthreads();
    }
    mine[pos] = x[pos];
}

void launch_fk20_transforms(G1Xyzz29 *pts, const uint8_t *roots, G1Xyzz29 *h_out, size_t n_blobs, hipStream_t st) {
    prof_launch("k_fk20_transforms", st, k_fk20_transforms, dim3((unsigned)n_blobs), dim3(kFk20Points), 0, pts, roots, fk20_beta29(), h_out);
}

// The finalize of a column call on this engine: msm.hip's k_finalize_compress with an index map in front, one
// lane per wanted proof. The points of the unwanted columns stay where the transforms left them
__global__ __launch_bounds__(64) void k_fk20_columns_compress(const G1Xyzz29 *__restrict__ pts, CellColumns cols, uint32_t c,
                                                              uint8_t *__restrict__ out48, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    __builtin_amdgcn_s_setprio(2);  // one inversion per lane, a pure latency chain at the end of the call
    uint8_t b[48];
    g1_compress(b, pts[(i / c) * kFk20Points + cols.k[i % c]]);
    uint32_t *o = (uint32_t *)(out48 + 48 * i);
#pragma unroll
    for (int k = 0; k < 12; k++)
        o[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
}

void launch_fk20_columns_compress(const G1Xyzz29 *pts, const CellColumns &cols, uint32_t c, uint8_t *out48, size_t n_blobs, hipStream_t st) {
    const size_t n = n_blobs * c;
    prof_launch("k_fk20_columns_compress", st, k_fk20_columns_compress, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, pts, cols, c, out48, n);
}

}  // namespace lwk
