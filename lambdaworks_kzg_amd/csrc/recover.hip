// recover.hip -- the kernels of EIP-7594 recover_cells_and_kzg_proofs in front of the cells pipeline (the
// pipeline is recover_api.hip): 64 .. 128 received cells of a blob -> its 4096 canonical coefficients in the workspace, where
// cells_from_coefficients (cells_api.hip) takes over.
//
// The problem factors through X^64. With p(X) = sum_{t<64} X^t P_t(X^64), deg P_t < 64, the interpolant of cell k on its coset is
// I_k = p mod (X^64 - c_k) and I_k[t] = P_t(c_k), c_k = w128^bitrev7(k): a blob is 64 independent erasure decodings of a polynomial of
// degree < 64 over the 128th roots of unity, all with the same erasure pattern. Per set, per (blob, cell) and per (blob, t), every
// step written once (the bodies below) behind two thin kernels: k_recover_* of the shared-set calls take the one set by value,
// k_recover_mixed_* of the mixed calls take set ids and find the sets' lists, masks and tables in device memory:
//
//  * setup: Zs(Y) = prod over the missing cells of (Y - c_k) at the 128 roots and at the coset 7 w128^i (inverted there), and
//    the powers of 7 the coset transforms scale by -- one 512-element table per set.
//  * interpolation: one wave per given cell. The range check of its 64 elements rides on the read; the 64-point inverse transform
//    over the coset (cell_interp.cuh, shared with the batch verification) gives I_k; I_k[t] Zs(c_k) goes to scratch [blob][t][bitrev7(k)].
//  * solve: one wave per (blob, t), 128 values in 4 KiB of LDS. The inverse transform of the 128 values (zero where the
//    cell is missing) is N_t = Q_t Zs, Q_t the interpolant of degree < num_cells through the given points; N_t / Zs on the coset
//    and back is Q_t. Its coefficients 64 .. 127 vanish exactly when a polynomial of degree < 4096 through the given cells exists;
//    otherwise the blob's status word is set. Q_t[m] is coefficient 64 m + t of the blob.
//
// Cell values are canonical integers and stay so through every step (a Montgomery-form factor times a raw value is the raw product),
// which is also the form the coefficients are wanted in.
#include "kernels.h"
#include "cell_interp.cuh"

namespace lwk {

namespace {

__device__ __forceinline__ uint32_t bitrev7(uint32_t q) { return __brev(q) >> 25; }

__device__ __forceinline__ bool position_given(const uint32_t *given, uint32_t q) { return (given[q >> 5] >> (q & 31u)) & 1u; }

// a 128-point decimation-in-time transform of buf in place, butterfly b of 64 per stage: bit-reversed order in, natural order out.
// tw: w4096^(+-e), e < 2048; w128^(+-j) is entry 32 j. Ends behind a barrier.
__device__ __forceinline__ void dft128(Fr *buf, const Fr *__restrict__ tw, uint32_t b) {
#pragma unroll 1
    for (int s = 0; s < 7; s++) {
        const uint32_t half = 1u << s, q = b & (half - 1);
        const uint32_t i0 = ((b >> s) << (s + 1)) + q, i1 = i0 + half;
        // w_(2 half)^q = w128^(q 64 / half)
        const Fr u = buf[i0], x = tw[32 * q * (64u >> s)] * buf[i1];
        buf[i0] = u + x;
        buf[i1] = u - x;
        __syncthreads();
    }
}

// buf[j] <- scale[j] buf[j] for the lane's two elements j = b, b + 64, stored in bit-reversed order for the next transform
__device__ __forceinline__ void scale_and_permute(Fr *buf, const Fr *__restrict__ scale, uint32_t b) {
    const Fr v0 = scale[b] * buf[b], v1 = scale[b + 64] * buf[b + 64];
    __syncthreads();
    buf[bitrev7(b)] = v0;
    buf[bitrev7(b + 64)] = v1;
    __syncthreads();
}

// ---- the three steps, each written once. A shared-set call hands its kernels the set by value and the context's one table; a mixed
// call hands them set ids, and the lists, masks and tables of its distinct sets are in device memory (the two wrappers of each below).

// The table of the set `given` is the mask of, by a workgroup of 128 lanes; lane q is position q, the root x_q = w128^q. tab (Montgomery
// form):
//   [q]        Zs(x_q) / 64        (the 1/64 of the cells' inverse transform rides here)
//   [128 + q]  1 / Zs(7 x_q)
//   [256 + q]  7^q / 128           (into the coset, with the scale of the inverse transform in front)
//   [384 + q]  7^-q / 128          (out of it, likewise)
// Zs is never expanded into coefficients: at most 64 factors per value, every lane its own two products. kWithList: lane k is also cell
// index k and the set's list goes to ks: ks[i] = the i-th given index, 0xff from the number of given cells on; the mask goes to mask_out.
template <bool kWithList>
__device__ __forceinline__ void recover_setup_body(const uint32_t *given, const Fr *__restrict__ tw_fwd, Fr *__restrict__ tab,
                                                   uint8_t *__restrict__ ks, uint32_t *__restrict__ mask_out) {
    __shared__ Fr root[kCellsPerBlob];
    __shared__ uint8_t has[kCellsPerBlob];   // by cell index (kWithList)
    const uint32_t q = threadIdx.x;
    const Fr x = q < 64 ? tw_fwd[32 * q] : neg(tw_fwd[32 * (q - 64)]);   // w128^64 = -1
    root[q] = x;
    if (kWithList) has[q] = position_given(given, bitrev7(q));
    __syncthreads();
    const Fr g = const_fr(kRecGenMont), gx = g * x;
    Fr zr = Fr::one(), zc = Fr::one();
    uint32_t rank = 0, count = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < (uint32_t)kCellsPerBlob; j++) {
        if (kWithList) {
            const uint32_t h = has[j];
            count += h;
            if (j < q) rank += h;
        }
        if (position_given(given, j)) continue;   // (the same for every lane)
        const Fr c = root[j];
        zr = zr * (x - c);
        zc = zc * (gx - c);
    }
    if (kWithList) {
        if (has[q]) ks[rank] = (uint8_t)q;
        if (q >= count) ks[q] = 0xff;
        if (q < (uint32_t)kCellsPerBlob / 32) mask_out[q] = given[q];
    }
    tab[q] = zr * const_fr(kRecInv64Mont);
    tab[128 + q] = inv_divsteps(zc);   // 7 x_q is no 128th root of unity: never zero
    Fr gp = Fr::one(), gip = Fr::one(), base = g, ibase = const_fr(kRecInvGenMont);
#pragma unroll 1
    for (int bit = 0; bit < 7; bit++) {
        if ((q >> bit) & 1u) {
            gp = gp * base;
            gip = gip * ibase;
        }
        base = sqr(base);
        ibase = sqr(ibase);
    }
    const Fr inv128 = const_fr(kRecInv128Mont);
    tab[256 + q] = gp * inv128;
    tab[384 + q] = gip * inv128;
}

// One wave (one workgroup) per given cell: blockIdx.x is the cell's place in `cells`, k its index, tab the table of its blob's set. Lane t
// reads element t, in the mode's byte order. An element that is not below r sets the blob's status word and counts as zero.
__device__ __forceinline__ void recover_interp_body(const uint4 *__restrict__ cells, uint32_t blob, uint32_t k, const Fr *__restrict__ tw_inv,
                                                    const Fr *__restrict__ tab, Fr *__restrict__ scratch, int32_t *__restrict__ status,
                                                    int bad_code, int le) {
    __shared__ Fr buf[kCellElems];
    const uint32_t t = threadIdx.x, q = bitrev7(k);
    const uint4 *e = cells + ((size_t)blockIdx.x * kCellElems + t) * 2;
    Fr x;
    element_limbs(x.l, e[0], e[1], le);
    const bool bad = raw_geq<8>(x.l, FrParams::MOD);
    if (bad) x = Fr::zero();
    if (__any(bad) && t == 0) status[blob] = bad_code;
    buf[t] = x;
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 6; s++) {
        if (t < 32) cell_idft64_stage(buf, tw_inv, s, t);
        __syncthreads();
    }
    // I_k[t] Zs(c_k): times h_k^-t, and Zs(c_k) / 64 from the table
    const Fr sc = cell_coeff_twist(tw_inv, k, t) * tab[q];
    scratch[((size_t)blob * kCellElems + t) * kCellsPerBlob + q] = sc * buf[t];
}

// One wave (one workgroup) per (blob, t): blockIdx.x = 64 blob + t; given and tab: the mask and the table of the blob's set. Lane b holds
// elements b and b + 64 wherever a lane owns elements.
__device__ __forceinline__ void recover_solve_body(const Fr *__restrict__ scratch, const uint32_t *given, const Fr *__restrict__ tw_fwd,
                                                   const Fr *__restrict__ tw_inv, const Fr *__restrict__ tab, uint4 *__restrict__ coeffs_raw,
                                                   int32_t *__restrict__ status, int bad_code) {
    __shared__ Fr buf[kCellsPerBlob];
    const uint32_t b = threadIdx.x, t = blockIdx.x % kCellElems, blob = blockIdx.x / kCellElems;
    const Fr *src = scratch + (size_t)blockIdx.x * kCellsPerBlob;
    // the slots of the missing cells were never written: they count as zero (Zs vanishes there)
    buf[bitrev7(b)] = position_given(given, b) ? src[b] : Fr::zero();
    buf[bitrev7(b + 64)] = position_given(given, b + 64) ? src[b + 64] : Fr::zero();
    __syncthreads();
    dft128(buf, tw_inv, b);                      // 128 N_t, N_t = Q_t Zs
    scale_and_permute(buf, tab + 256, b);        // N_t[j] 7^j
    dft128(buf, tw_fwd, b);                      // N_t(7 w128^i)
    scale_and_permute(buf, tab + 128, b);        // Q_t(7 w128^i)
    dft128(buf, tw_inv, b);                      // 128 Q_t[j] 7^j
    const Fr lo = tab[384 + b] * buf[b], hi = tab[384 + b + 64] * buf[b + 64];
    if (__any(!hi.is_zero()) && b == 0) status[blob] = bad_code;
    const size_t slot = (size_t)blob * kBlobElems + (size_t)kCellElems * b + t;
    coeffs_raw[2 * slot] = make_uint4(lo.l[0], lo.l[1], lo.l[2], lo.l[3]);
    coeffs_raw[2 * slot + 1] = make_uint4(lo.l[4], lo.l[5], lo.l[6], lo.l[7]);
}

}  // namespace

// ---- the shared-set form: the set by value, one table

// one workgroup of 128 lanes per call
__global__ __launch_bounds__(128) void k_recover_setup(RecoverSet set, const Fr *__restrict__ tw_fwd, Fr *__restrict__ tab) {
    recover_setup_body<false>(set.given, tw_fwd, tab, nullptr, nullptr);
}

// blockIdx.x = blob * num_cells + i for the i-th given cell of a blob
__global__ __launch_bounds__(64) void k_recover_interp(const uint4 *__restrict__ cells, RecoverSet set, uint32_t num_cells,
                                                       const Fr *__restrict__ tw_inv, const Fr *__restrict__ tab, Fr *__restrict__ scratch,
                                                       int32_t *__restrict__ status, int bad_code, int le) {
    recover_interp_body(cells, blockIdx.x / num_cells, set.k[blockIdx.x % num_cells], tw_inv, tab, scratch, status, bad_code, le);
}

__global__ __launch_bounds__(64) void k_recover_solve(const Fr *__restrict__ scratch, RecoverSet set, const Fr *__restrict__ tw_fwd,
                                                      const Fr *__restrict__ tw_inv, const Fr *__restrict__ tab, uint4 *__restrict__ coeffs_raw,
                                                      int32_t *__restrict__ status, int bad_code) {
    recover_solve_body(scratch, set.given, tw_fwd, tw_inv, tab, coeffs_raw, status, bad_code);
}

// ---- the mixed form: every blob its own set (recover_api.hip: lwkzg_recover_cells_and_kzg_proofs_mixed). The sets reach the device as
// 128-bit masks by value to the setup, which leaves everything else a set needs in device memory, and the blobs' set ids and cell
// offsets by value to the other two. Nothing here reads host memory or a buffer the host writes.

// one workgroup of 128 lanes per distinct set: block s makes set first + s from masks.given[s]
__global__ __launch_bounds__(128) void k_recover_mixed_setup(RecoverMasks masks, uint32_t first, const Fr *__restrict__ tw_fwd,
                                                             Fr *__restrict__ tabs, uint8_t *__restrict__ ks, uint32_t *__restrict__ givens) {
    const size_t set = (size_t)first + blockIdx.x;
    recover_setup_body<true>(masks.given[blockIdx.x], tw_fwd, tabs + set * kRecoverTabElems, ks + set * kCellsPerBlob,
                             givens + set * (kCellsPerBlob / 32));
}

// blockIdx.x is the cell's place among the group's cells, its blob the last one of the group whose cells start at or before it (every
// blob has cells, so cell0 ascends strictly)
__global__ __launch_bounds__(64) void k_recover_mixed_interp(const uint4 *__restrict__ cells, RecoverGroup grp, uint32_t n_blobs,
                                                             const Fr *__restrict__ tw_inv, const Fr *__restrict__ tabs,
                                                             const uint8_t *__restrict__ ks, Fr *__restrict__ scratch,
                                                             int32_t *__restrict__ status, int bad_code, int le) {
    uint32_t blob = 0, end = n_blobs;   // cell0[blob] <= blockIdx.x < cell0[end] (the group's cell count where end = n_blobs)
    while (end - blob > 1) {
        const uint32_t mid = (blob + end) >> 1;
        if (grp.cell0[mid] <= blockIdx.x) blob = mid;
        else end = mid;
    }
    const size_t set = grp.set[blob];
    recover_interp_body(cells, blob, ks[set * kCellsPerBlob + blockIdx.x - grp.cell0[blob]], tw_inv, tabs + set * kRecoverTabElems, scratch,
                        status, bad_code, le);
}

__global__ __launch_bounds__(64) void k_recover_mixed_solve(const Fr *__restrict__ scratch, RecoverGroup grp, const Fr *__restrict__ tw_fwd,
                                                            const Fr *__restrict__ tw_inv, const Fr *__restrict__ tabs,
                                                            const uint32_t *__restrict__ givens, uint4 *__restrict__ coeffs_raw,
                                                            int32_t *__restrict__ status, int bad_code) {
    const size_t set = grp.set[blockIdx.x / kCellElems];
    recover_solve_body(scratch, givens + set * (kCellsPerBlob / 32), tw_fwd, tw_inv, tabs + set * kRecoverTabElems, coeffs_raw, status,
                       bad_code);
}

void launch_recover_setup(const RecoverSet &set, const Fr *tw_fwd, Fr *tab, hipStream_t st) {
    prof_launch("k_recover_setup", st, k_recover_setup, dim3(1), dim3(kCellsPerBlob), 0, set, tw_fwd, tab);
}

void launch_recover_coefficients(const uint8_t *cells, const RecoverSet &set, size_t num_cells, const Fr *tw_fwd, const Fr *tw_inv, const Fr *tab,
                                 Fr *scratch, uint32_t *coeffs_raw, int32_t *status, int bad_code, int le, size_t n_blobs, hipStream_t st) {
    prof_launch("k_recover_interp", st, k_recover_interp, dim3((unsigned)(n_blobs * num_cells)), dim3(kCellElems), 0, (const uint4 *)cells, set,
                (uint32_t)num_cells, tw_inv, tab, scratch, status, bad_code, le);
    prof_launch("k_recover_solve", st, k_recover_solve, dim3((unsigned)(n_blobs * kCellElems)), dim3(kCellElems), 0, (const Fr *)scratch, set, tw_fwd,
                tw_inv, tab, (uint4 *)coeffs_raw, status, bad_code);
}

void launch_recover_mixed_setup(const RecoverMasks &masks, size_t first, size_t n_sets, const Fr *tw_fwd, const RecoverSetsDev &dev, hipStream_t st) {
    prof_launch("k_recover_mixed_setup", st, k_recover_mixed_setup, dim3((unsigned)n_sets), dim3(kCellsPerBlob), 0, masks, (uint32_t)first, tw_fwd,
                dev.tab, dev.k, dev.given);
}

void launch_recover_mixed_coefficients(const uint8_t *cells, const RecoverGroup &g, size_t n_cells, const Fr *tw_fwd, const Fr *tw_inv,
                                       const RecoverSetsDev &dev, Fr *scratch, uint32_t *coeffs_raw, int32_t *status, int bad_code, int le,
                                       size_t n_blobs, hipStream_t st) {
    prof_launch("k_recover_mixed_interp", st, k_recover_mixed_interp, dim3((unsigned)n_cells), dim3(kCellElems), 0, (const uint4 *)cells, g,
                (uint32_t)n_blobs, tw_inv, (const Fr *)dev.tab, (const uint8_t *)dev.k, scratch, status, bad_code, le);
    prof_launch("k_recover_mixed_solve", st, k_recover_mixed_solve, dim3((unsigned)(n_blobs * kCellElems)), dim3(kCellElems), 0, (const Fr *)scratch,
                g, tw_fwd, tw_inv, (const Fr *)dev.tab, (const uint32_t *)dev.given, (uint4 *)coeffs_raw, status, bad_code);
}

}  // namespace lwk
