// cells_verify.hip -- the kernels of EIP-7594 verify_cell_kzg_proof_batch that the blob batch verification does not already have
// (the pipeline is cells_verify_api.hip). For n items (C_i, k_i, cell_i, pi_i) over m distinct commitments:
//
//  * Digests: d_i = SHA-256(le64(row_i) | le64(k_i) | cell_i | pi_i), 2112 bytes = 33 blocks and the padding block, one lane per
//    cell, every cell in parallel; the range check of the cell's 64 elements rides on the same read.
//  * Scalars behind r: a_i = r^i from the table of r^(2^k), b_i = a_i c_{k_i} (c_k = w128^bitrev7(k), a forward twiddle or its
//    negative), both split as lo + hi z^2 for k_vmsm_accumulate; the weights w_j = sum_{row_i = j} a_i of the distinct commitments
//    in the same form.
//  * Column sums and interpolation: S_k[t] = sum_{k_i = k} a_i cell_i[t], a 64-point inverse transform of S_k in LDS (the cell's
//    elements are the evaluations on the coset h_k <w64> in bit-reversed order: exactly the order a decimation-in-time transform
//    consumes), coefficient t scaled by h_k^-t / 64, and the 128 columns summed into the 64 coefficients of I(X) = sum a_i I_i(X),
//    written as canonical limbs into one 4096-scalar MSM slot whose other 4032 scalars are zero. The two kernels run on a grid of
//    (.., groups): a call of g groups (cells_verify_groups.hip) is the same launches with one interpolant and one slot per group,
//    and the batch is one group.
//
// Items are grouped by row and by column on the host (a counting sort over the indices it holds anyway) or, for an asynchronous
// verifier, by cell_group.hip on the device: perm_* lists the items of group g at [off[g], off[g + 1]), in any order.
#include "kernels.h"
#include "cell_interp.cuh"
#include "sha256_round.cuh"

namespace lwk {

namespace {

__device__ __forceinline__ void absorb(uint32_t w[16], int j, const uint4 &c) {
    w[4 * j] = __builtin_bswap32(c.x);
    w[4 * j + 1] = __builtin_bswap32(c.y);
    w[4 * j + 2] = __builtin_bswap32(c.z);
    w[4 * j + 3] = __builtin_bswap32(c.w);
}

}  // namespace

// ---- the per-cell transcript digests and the range check -------------------------------------------------------------------------
// The message as 132 16-byte chunks: 0 = le64(row) | le64(k), 1 .. 128 = the cell, 129 .. 131 = the proof; block b holds chunks
// 4 b .. 4 b + 3, so an element (cell chunks 2 e, 2 e + 1 = message chunks 2 e + 1, 2 e + 2) is complete at every even message chunk
// from 2 to 128. digests: 32 bytes per item; status[i] = bad_code where an element is not below r.
__global__ __launch_bounds__(64) void k_cellv_digests(const uint4 *__restrict__ cells, const uint4 *__restrict__ proofs,
                                                      const uint32_t *__restrict__ rows, const uint64_t *__restrict__ idx,
                                                      uint32_t *__restrict__ digests, int32_t *__restrict__ status, int bad_code, int le,
                                                      uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 *cell = cells + (size_t)2 * kCellElems * i;
    const uint4 *pf = proofs + (size_t)3 * i;
    const uint64_t k = idx[i];
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    uint32_t w[16], t[8];
    bool bad = false;
    uint4 prev = make_uint4(rows[i], 0u, (uint32_t)k, (uint32_t)(k >> 32));
    // block 0: the header and cell chunks 0 .. 2
    absorb(w, 0, prev);
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const uint4 c = cell[j - 1];
        absorb(w, j, c);
        if (j == 2) {
            element_limbs(t, prev, c, le);
            bad |= raw_geq<8>(t, FrParams::MOD);
        }
        prev = c;
    }
    sha256_compress(h, w);
    // blocks 1 .. 31: cell chunks 4 b - 1 .. 4 b + 2
#pragma unroll 1
    for (int b = 1; b < 32; b++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint4 c = cell[4 * b - 1 + j];
            absorb(w, j, c);
            if (!(j & 1)) {
                element_limbs(t, prev, c, le);
                bad |= raw_geq<8>(t, FrParams::MOD);
            }
            prev = c;
        }
        sha256_compress(h, w);
    }
    // block 32: the last cell chunk and the proof
    {
        const uint4 c = cell[2 * kCellElems - 1];
        absorb(w, 0, c);
        element_limbs(t, prev, c, le);
        bad |= raw_geq<8>(t, FrParams::MOD);
#pragma unroll
        for (int j = 1; j < 4; j++) absorb(w, j, pf[j - 1]);
        sha256_compress(h, w);
    }
    // padding: 0x80, zeros, the length in bits (2112 * 8) big-endian
    w[0] = 0x80000000u;
#pragma unroll
    for (int j = 1; j < 15; j++) w[j] = 0;
    w[15] = 2112u * 8u;
    sha256_compress(h, w);
    uint4 *out = (uint4 *)(digests + 8 * (size_t)i);
    out[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
    out[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
    if (bad) status[i] = bad_code;
}

void launch_cellv_digests(const uint8_t *cells, const uint8_t *proofs48, const uint32_t *rows, const uint64_t *idx, uint8_t *digests32,
                          int32_t *status, int bad_code, int le, size_t n, hipStream_t st) {
    prof_launch("k_cellv_digests", st, k_cellv_digests, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (const uint4 *)cells, (const uint4 *)proofs48,
                rows, idx, (uint32_t *)digests32, status, bad_code, le, (uint32_t)n);
}

// ---- behind r: a_i = r^i, b_i = a_i c_{k_i} ------------------------------------------------------------------------------------------
// pw as k_vmsm_scalars takes it (r^(2^k), k < 32, then r^first; the cell batch starts at r^0). a_mont keeps a_i in Montgomery form
// for the weights and the column sums; sc_a / sc_b are the split forms of a_i and b_i (cell_interp.cuh: cell_item_scalars, which
// k_cellg_scalars runs too, on its group's table).
__global__ __launch_bounds__(64) void k_cellv_scalars(const Fr *__restrict__ pw, const uint64_t *__restrict__ idx, const Fr *__restrict__ tw_fwd,
                                                      Fr *__restrict__ a_mont, uint32_t *__restrict__ sc_a, uint32_t *__restrict__ sc_b,
                                                      uint32_t n, const uint32_t *__restrict__ skip) {
    if (skip && *skip) return;  // a rejected batch of an asynchronous verifier (cells_verify_async.hip): its indices are unchecked
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cell_item_scalars(pw, i, i, idx, tw_fwd, a_mont, sc_a, sc_b);
}

// w_j = sum of a_i over the items of row j, one wave per row. m_dev (optional): the number of rows where only the device knows it -- the
// launch then covers n rows and the workgroups at j >= *m_dev leave (all of a workgroup, before its first barrier, as under skip)
__global__ __launch_bounds__(64) void k_cellv_row_weights(const Fr *__restrict__ a_mont, const uint32_t *__restrict__ perm_row,
                                                          const uint32_t *__restrict__ row_off, uint32_t *__restrict__ sc_c,
                                                          const uint32_t *__restrict__ m_dev, const uint32_t *__restrict__ skip) {
    __shared__ Fr sh[64];
    if (skip && *skip) return;
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    if (m_dev && j >= *m_dev) return;
    const uint32_t lo = row_off[j], hi = row_off[j + 1];
    Fr acc = Fr::zero();
    for (uint32_t s = lo + t; s < hi; s += 64) acc = acc + a_mont[perm_row[s]];
    sh[t] = acc;
    __syncthreads();
    for (int d = 32; d >= 1; d >>= 1) {
        if ((int)t < d) sh[t] = sh[t] + sh[t + d];
        __syncthreads();
    }
    if (t != 0) return;
    uint32_t raw[8];
    fe_to_raw<FrParams>(raw, sh[0]);
    store_split(sc_c, j, raw);
}

void launch_cellv_scalars(const Fr *pw, const uint64_t *idx, const Fr *tw_fwd, Fr *a_mont, uint32_t *sc_a, uint32_t *sc_b,
                          const uint32_t *perm_row, const uint32_t *row_off, uint32_t *sc_c, size_t n, size_t m, hipStream_t st,
                          const uint32_t *m_dev, const uint32_t *skip) {
    prof_launch("k_cellv_scalars", st, k_cellv_scalars, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, pw, idx, tw_fwd, a_mont, sc_a, sc_b,
                (uint32_t)n, skip);
    launch_cellv_row_weights(a_mont, perm_row, row_off, sc_c, m_dev ? n : m, st, m_dev, skip);
}

void launch_cellv_row_weights(const Fr *a_mont, const uint32_t *perm_row, const uint32_t *row_off, uint32_t *sc_c, size_t rows, hipStream_t st,
                              const uint32_t *m_dev, const uint32_t *skip) {
    if (rows == 0) return;
    prof_launch("k_cellv_row_weights", st, k_cellv_row_weights, dim3((unsigned)rows), dim3(64), 0, a_mont, perm_row, row_off, sc_c, m_dev, skip);
}

// ---- the fault words of an asynchronous verifier ------------------------------------------------------------------------------------
// The validation marks item i and distinct commitment i in ONE status word. A verifier reports the lowest item at fault, and a bad
// commitment counts where it was first seen, so the two are told apart here: fault[i] (on entry the digests' word: a cell element not
// below r) also takes proof i's verdict, fault[n + j] is distinct commitment j's (the padding behind the m-th is infinity: never bad).
__global__ __launch_bounds__(256) void k_cellv_fault_words(int32_t *__restrict__ fault, const int32_t *__restrict__ kind_p,
                                                           const int32_t *__restrict__ kind_c, int bad_code, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (kind_p[i] == 2) fault[i] = bad_code;
    fault[n + i] = kind_c[i] == 2 ? bad_code : 0;
}

void launch_cellv_fault_words(int32_t *fault, const int32_t *kind_p, const int32_t *kind_c, int bad_code, size_t n, hipStream_t st) {
    prof_launch("k_cellv_fault_words", st, k_cellv_fault_words, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fault, kind_p, kind_c, bad_code,
                (uint32_t)n);
}

hipError_t launch_cellv_first_visit(const uint8_t *cells, const uint64_t *idx, const uint32_t *rows, const PointSet &set_p, const PointSet &set_c,
                                    uint8_t *digests32, int32_t *fault, int32_t *status, int bad_code, int le, size_t n, hipStream_t st,
                                    hipEvent_t digests_done) {
    hipError_t e = hipMemsetAsync(fault, 0, 4 * n, st);   // (the digests write a word only where an element is out of range)
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, 4 * n, st);
    if (e != hipSuccess) return e;
    launch_cellv_digests(cells, set_p.in48, rows, idx, digests32, fault, bad_code, le, n, st);
    if (digests_done) e = hipEventRecord(digests_done, st);
    launch_decompress_points(set_p, &set_c, n, st);
    launch_subgroup_canon(set_p, &set_c, status, bad_code, n, st, false, true);
    launch_cellv_fault_words(fault, set_p.kind, set_c.kind, bad_code, n, st);
    return e;
}

// ---- behind r: the column sums, their interpolation, and the 64 coefficients of I(X) ------------------------------------------------
// One workgroup per (column k, group first + blockIdx.y), four waves: wave v sums every fourth item of the column (lane t = element t
// of the cell; a wave reads a cell's 2 KiB in one pass), the four partial sums meet in LDS, and 32 lanes run the six stages of the
// 64-point decimation-in-time inverse transform in place. The cell's values are canonical integers and stay so: a Montgomery product
// of a Montgomery-form factor (a_i, a twiddle, the scale) with a raw value is the raw product. col_off: the group's column k is list
// 128 (first + blockIdx.y) + k. colcoef[(128 blockIdx.y + k) 64 + t]: coefficient t of the column's share of the group's interpolant,
// canonical limbs (zero for a column nobody sampled). flag (nullptr: nobody is flagged): one word per group -- a batch's skip word
// (one group, first = 0), a grouped call's flags.
__global__ __launch_bounds__(256) void k_cellv_columns(const uint4 *__restrict__ cells, const Fr *__restrict__ a_mont,
                                                       const uint32_t *__restrict__ perm_col, const uint32_t *__restrict__ col_off,
                                                       const uint32_t *__restrict__ flag, const Fr *__restrict__ tw_inv,
                                                       Fr *__restrict__ colcoef, int le, uint32_t first) {
    __shared__ Fr part[4][kCellElems];
    __shared__ Fr buf[kCellElems];
    const uint32_t k = blockIdx.x, jj = blockIdx.y, j = first + jj, t = threadIdx.x & 63u, v = threadIdx.x >> 6;
    if (flag && flag[j]) return;  // (the whole workgroup, before its first barrier; k_cellv_coeffs then reads nothing of its scratch)
    Fr *out = colcoef + ((size_t)kCellsPerBlob * jj + k) * kCellElems;
    const uint32_t lo = col_off[(size_t)kCellsPerBlob * j + k], hi = col_off[(size_t)kCellsPerBlob * j + k + 1];
    if (lo == hi) {   // (the same for the whole workgroup: no barrier is left behind)
        if (v == 0) out[t] = Fr::zero();
        return;
    }
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t s = lo + v; s < hi; s += 4) {
        const uint32_t i = perm_col[s];
        const uint4 *e = cells + ((size_t)kCellElems * i + t) * 2;
        Fr x;
        element_limbs(x.l, e[0], e[1], le);
        acc = acc + a_mont[i] * x;
    }
    part[v][t] = acc;
    __syncthreads();
    if (v == 0) buf[t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 6; s++) {
        if (threadIdx.x < 32) cell_idft64_stage(buf, tw_inv, s, threadIdx.x);
        __syncthreads();
    }
    if (v != 0) return;
    out[t] = cell_coeff_scale(tw_inv, k, t) * buf[t];   // times h_k^-t / 64
}

// scalar t of MSM slot blockIdx.y (group first + blockIdx.y): the sum of the 128 columns' coefficient t for t < 64, zero above; all 4096
// zero for a flagged group (the engine's launch set behind this kernel takes no flag, so its slot is defined either way)
__global__ __launch_bounds__(256) void k_cellv_coeffs(const Fr *__restrict__ colcoef, const uint32_t *__restrict__ flag, Fr *__restrict__ slots,
                                                      uint32_t first) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, jj = blockIdx.y;
    Fr acc = Fr::zero();
    if (t < (uint32_t)kCellElems && !(flag && flag[first + jj])) {
        const Fr *cc = colcoef + (size_t)kCellsPerBlob * kCellElems * jj;
#pragma unroll 1
        for (int k = 0; k < kCellsPerBlob; k++) acc = acc + cc[kCellElems * k + t];
    }
    slots[(size_t)kBlobElems * jj + t] = acc;
}

void launch_cellv_interpolant(const uint8_t *cells, const Fr *a_mont, const uint32_t *perm_col, const uint32_t *col_off, const Fr *tw_inv,
                              Fr *colcoef, uint32_t *slot_raw, int le, hipStream_t st, const uint32_t *flag, size_t first, size_t groups) {
    prof_launch("k_cellv_columns", st, k_cellv_columns, dim3(kCellsPerBlob, (unsigned)groups), dim3(256), 0, (const uint4 *)cells, a_mont,
                perm_col, col_off, flag, tw_inv, colcoef, le, (uint32_t)first);
    prof_launch("k_cellv_coeffs", st, k_cellv_coeffs, dim3(kBlobElems / 256, (unsigned)groups), dim3(256), 0, (const Fr *)colcoef, flag,
                (Fr *)slot_raw, (uint32_t)first);
}

}  // namespace lwk
