// cells.hip -- the kernels of EIP-7594 cells and cell proofs around the MSM (the pipeline is cells_api.hip).
//
//  * Extension: the 4096 coefficients of a blob -> its 8192 evaluations on the extended domain D[j] = w8192^bitrev13(j), i.e. the
//    4096 evaluations of p(X) (elements 0 .. 4095, cells 0 .. 63) and of p(w8192 X) (elements 4096 .. 8191, cells 64 .. 127), each
//    half in bit-reversed order. Two forward transforms per blob through fr_ops.hip's k_ntt4096 (Montgomery in, Montgomery out,
//    natural order in and out); the kernels on either side do the scaling by w8192^i, the bit-reversal permutations, the entry into
//    and the exit from Montgomery form and the serialisation in the mode's byte order.
//  * Quotients: q_k = p div (X^64 - c_k), c_k = w128^bitrev7(k), by the binomial recurrence q[j] = p[j + 64] + c_k q[j + 64] from
//    the top down, written as canonical limbs straight into the MSM's scalar slots.
//  * A call for c of the 128 columns takes the list by value in the extension's exit and in the quotients:
//    k_cells_extend_out_columns and k_cells_quotients_columns, each one body with its twin that knows no list.
#include "kernels.h"

namespace lwk {

// w8192 R^2 mod r (w8192 = 7^((r-1)/8192), R = 2^256), canonical limbs: the Montgomery product of a raw value x with it is w8192 x in
// Montgomery form. w8192^2 is fr_ops.hip's kOmegaRaw (tests/test_cells_cpu.py holds both against Python's pow).
__device__ __constant__ uint32_t kOmega8192R2[8] = {0x31147553u, 0x3d081affu, 0x3c4bc938u, 0x55e2de4eu,
                                                    0xf2fa8218u, 0x9a8b2ebcu, 0xf306266au, 0x28ebd06eu};

__device__ __forceinline__ Fr load_raw(const uint4 *p, size_t i) {
    const uint4 lo = p[2 * i], hi = p[2 * i + 1];
    Fr v;
    v.l[0] = lo.x, v.l[1] = lo.y, v.l[2] = lo.z, v.l[3] = lo.w;
    v.l[4] = hi.x, v.l[5] = hi.y, v.l[6] = hi.z, v.l[7] = hi.w;
    return v;
}
__device__ __forceinline__ void store_raw(uint4 *p, size_t i, const uint32_t *s) {
    p[2 * i] = make_uint4(s[0], s[1], s[2], s[3]);
    p[2 * i + 1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// Entry: lane g is position `pos` of transform t = 2 b + h; it takes coefficient i = bitrev12(pos) of blob b (the transform is
// decimation in time: bit-reversed input, natural output) and writes it in Montgomery form, times w8192^i when h = 1:
// w8192^i = w8192^(i mod 2) w^(i >> 1), the context's forward twiddles (w^k, k < 2048) and the constant above. Reads gather, writes
// are contiguous.
__global__ __launch_bounds__(256) void k_cells_extend_in(const uint4 *__restrict__ coeffs_raw, const Fr *__restrict__ tw_fwd,
                                                         Fr *__restrict__ out, size_t n) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const size_t t = g / kBlobElems;
    const uint32_t pos = (uint32_t)(g % kBlobElems), i = __brev(pos) >> 20;
    const Fr c = load_raw(coeffs_raw, (t >> 1) * kBlobElems + i);
    Fr k;
    if (t & 1) {
        const bool odd = i & 1;
#pragma unroll
        for (int j = 0; j < 8; j++) k.l[j] = odd ? kOmega8192R2[j] : FrParams::R2[j];
        out[g] = k * (tw_fwd[i >> 1] * c);   // (w^(i>>1) R) c / R = raw; then (w8192^(i&1) R^2) x / R = Montgomery
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) k.l[j] = FrParams::R2[j];
        out[g] = k * c;
    }
}

// Exit: lane g is element e of blob b's 8192 (cell e / 64, slot e mod 64); it reads evaluation bitrev12(e mod 4096) of transform
// 2 b + (e >= 4096) and writes its 32 bytes, little-endian (le) or big-endian. Reads gather, writes are contiguous.
// (the body: element e of blob b to output element g; both exit kernels are this)
__device__ __forceinline__ void cells_extend_store(const Fr *__restrict__ evals, uint4 *__restrict__ cells, int le, size_t b, uint32_t e, size_t g) {
    const uint32_t h = e / kBlobElems, j = __brev(e % kBlobElems) >> 20;
    uint32_t s[8];
    fe_to_raw<FrParams>(s, evals[(2 * b + h) * kBlobElems + j]);
    if (le) {
        store_raw(cells, g, s);
    } else {
        cells[2 * g] = make_uint4(__builtin_bswap32(s[7]), __builtin_bswap32(s[6]), __builtin_bswap32(s[5]), __builtin_bswap32(s[4]));
        cells[2 * g + 1] = make_uint4(__builtin_bswap32(s[3]), __builtin_bswap32(s[2]), __builtin_bswap32(s[1]), __builtin_bswap32(s[0]));
    }
}

__global__ __launch_bounds__(256) void k_cells_extend_out(const Fr *__restrict__ evals, uint4 *__restrict__ cells, int le, size_t n) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    cells_extend_store(evals, cells, le, g / (2 * kBlobElems), (uint32_t)(g % (2 * kBlobElems)), g);
}

// The exit of a call that wants c columns: lane g is slot t of the blob's i-th wanted cell, output element
// g = 64 (c b + i) + t, and reads what the exit above reads for element 64 cols.k[i] + t. The list comes by value: no buffer to keep
__global__ __launch_bounds__(256) void k_cells_extend_out_columns(const Fr *__restrict__ evals, uint4 *__restrict__ cells, int le,
                                                                  CellColumns cols, uint32_t c, size_t n) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const size_t cell = g / kCellElems;
    const uint32_t i = (uint32_t)(cell % c), t = (uint32_t)(g % kCellElems);
    cells_extend_store(evals, cells, le, cell / c, (uint32_t)kCellElems * cols.k[i] + t, g);
}

void launch_cells_extend(const uint32_t *coeffs_raw, const Fr *tw_fwd, const Fr28 *tw28_fwd, Fr *scratch, Fr *scratch2, uint8_t *cells,
                         int le, size_t n_blobs, hipStream_t st, const CellColumns *cols, uint32_t c) {
    const size_t n = 2 * n_blobs * kBlobElems;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    prof_launch("k_cells_extend_in", st, k_cells_extend_in, dim3(blocks), dim3(256), 0, (const uint4 *)coeffs_raw, tw_fwd, scratch, n);
    launch_ntt4096(scratch, scratch2, tw28_fwd, 0, 2 * n_blobs, st);
    if (cols) {   // the transforms stay whole; only the wanted cells leave
        const size_t n_out = n_blobs * c * kCellElems;
        prof_launch("k_cells_extend_out_columns", st, k_cells_extend_out_columns, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0,
                    (const Fr *)scratch2, (uint4 *)cells, le, *cols, c, n_out);
        return;
    }
    prof_launch("k_cells_extend_out", st, k_cells_extend_out, dim3(blocks), dim3(256), 0, (const Fr *)scratch2, (uint4 *)cells, le, n);
}

// One lane per (blob, cell k, t = j mod 64): a wave is one (blob, cell) and reads 64 consecutive coefficients / writes 64 consecutive
// quotient coefficients (2 KiB each) per step. q_k has degree < 4032; slots 4032 .. 4095 of its scalar set are zero. Coefficients
// and quotient are raw canonical integers: the Montgomery product of c_k R (the twiddle w^(32 bitrev7(k)), negated from the
// table's upper half: w^2048 = -1) with a raw q is c_k q, raw again. 62 products per lane.
// (the body: lane t of the wave of cell k; p the blob's coefficients, q the scalar set. Both quotient kernels are this)
__device__ __forceinline__ void cells_quotient(const uint4 *__restrict__ p, const Fr *__restrict__ tw_fwd, uint4 *__restrict__ q, uint32_t k,
                                               uint32_t t) {
    const uint32_t e = 32 * (__brev(k) >> 25);
    const Fr ck = e < kBlobElems / 2 ? tw_fwd[e] : neg(tw_fwd[e - kBlobElems / 2]);
    constexpr uint32_t kTop = kBlobElems - kCellElems;   // 4032
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    store_raw(q, kTop + t, zero);
    Fr acc = load_raw(p, kTop + t);
    store_raw(q, kTop - kCellElems + t, acc.l);
    for (int j = (int)(kTop - 2 * kCellElems + t); j >= 0; j -= kCellElems) {
        acc = load_raw(p, j + kCellElems) + ck * acc;
        store_raw(q, j, acc.l);
    }
}

__global__ __launch_bounds__(256) void k_cells_quotients(const uint4 *__restrict__ coeffs_raw, const Fr *__restrict__ tw_fwd,
                                                         uint4 *__restrict__ quot_raw, size_t n_cells) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t cell = g / kCellElems;
    if (cell >= n_cells) return;
    cells_quotient(coeffs_raw + (cell / kCellsPerBlob) * kBlobElems * 2, tw_fwd, quot_raw + cell * kBlobElems * 2,
                   (uint32_t)(cell % kCellsPerBlob), (uint32_t)(g % kCellElems));
}

// The quotients of a call that wants c columns: one wave per (blob, i < c), k = cols.k[i], into scalar set c blob + i
__global__ __launch_bounds__(256) void k_cells_quotients_columns(const uint4 *__restrict__ coeffs_raw, const Fr *__restrict__ tw_fwd,
                                                                 uint4 *__restrict__ quot_raw, CellColumns cols, uint32_t c, size_t n_sets) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t set = g / kCellElems;
    if (set >= n_sets) return;
    cells_quotient(coeffs_raw + (set / c) * kBlobElems * 2, tw_fwd, quot_raw + set * kBlobElems * 2, cols.k[set % c],
                   (uint32_t)(g % kCellElems));
}

void launch_cells_quotients(const uint32_t *coeffs_raw, const Fr *tw_fwd, uint32_t *quot_raw, size_t n_cells, hipStream_t st) {
    const size_t n = n_cells * kCellElems;
    prof_launch("k_cells_quotients", st, k_cells_quotients, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint4 *)coeffs_raw, tw_fwd,
                (uint4 *)quot_raw, n_cells);
}

void launch_cells_quotients_columns(const uint32_t *coeffs_raw, const Fr *tw_fwd, uint32_t *quot_raw, const CellColumns &cols, uint32_t c,
                                    size_t n_blobs, hipStream_t st) {
    const size_t n_sets = n_blobs * c, n = n_sets * kCellElems;
    prof_launch("k_cells_quotients_columns", st, k_cells_quotients_columns, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                (const uint4 *)coeffs_raw, tw_fwd, (uint4 *)quot_raw, cols, c, n_sets);
}

}  // namespace lwk
