// msm.hip -- batched fixed-base Pippenger G1 MSM for gfx950 (MI355X).
//
// Replaces lambdaworks_math::msm::pippenger::msm as reached from KZG::commit / KZG::open
// (call sites /root/reference/src/lib.rs:242,270,329,394) for 4096-term MSMs over the trusted
// setup. Not a port of the upstream loop (one sequential window at a time, projective adds into a
// heap Vec): see plan.h for the shape. Stages, each its own kernel, all blobs of a batch at once:
//
//   k_parse_*          blob bytes -> canonical 256-bit scalars                (HBM streaming, 16 B/lane)
//   k_digit_sort       signed 13-bit digits, LDS histogram + wave64 prefix sum, counting-sort the
//                      (window, point, sign) entries by bucket; also orders buckets by population
//   k_bucket_accumulate one lane per bucket, XYZZ accumulator in VGPRs, affine table point gathered
//                      from the Infinity-Cache-resident table (96 B contiguous per lane)
//   k_bucket_reduce    sum_k k*B_k per blob: per-lane running sums + LDS suffix scan / tree
//   k_finalize_compress one inversion per blob, ZCash compression
//
// The work is integer-ALU bound (about 1e6 381-bit Montgomery products per blob against 0.5 MB
// of algorithmic traffic), so the kernels are organised around VGPR residency and wave balance,
// not around HBM bandwidth; DESIGN.md has the arithmetic.
#include "kernels.h"
#include "knobs.h"

#include <stdlib.h>

namespace lwk {

// ------------------------------------------------------------------------------------------------
// scalar ingest

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// one lane per field element; 32 B in (2 x 16 B), 32 B out
// (zero / zero_words, r06: words this launch clears on its way -- a one-blob call's hand-off counters, instead of a fill launch of their own;
// zero2: a second region -- a batch's status words and the redo flags of its MSM, which were a fill launch each)
__global__ __launch_bounds__(256) void k_parse_be_reduce(const uint4 *__restrict__ in, uint4 *__restrict__ out,
                                                         size_t n_elems, uint32_t *__restrict__ zero, uint32_t zero_words,
                                                         uint32_t *__restrict__ zero2, uint32_t zero2_words) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < zero_words) zero[i] = 0u;
    if (i < zero2_words) zero2[i] = 0u;
    if (i >= n_elems) return;
    uint4 hi = in[2 * i], lo = in[2 * i + 1];  // big-endian: first 16 bytes are the most significant
    uint32_t s[8];
    s[7] = bswap32(hi.x);
    s[6] = bswap32(hi.y);
    s[5] = bswap32(hi.z);
    s[4] = bswap32(hi.w);
    s[3] = bswap32(lo.x);
    s[2] = bswap32(lo.y);
    s[1] = bswap32(lo.z);
    s[0] = bswap32(lo.w);
    // reduce mod r: 2^256 < 3r, so at most two subtractions
#pragma unroll
    for (int k = 0; k < 2; k++) {
        uint32_t d[8];
        uint32_t br = raw_sub<8>(d, s, FrParams::MOD);
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = br ? s[j] : d[j];
    }
    out[2 * i] = make_uint4(s[0], s[1], s[2], s[3]);
    out[2 * i + 1] = make_uint4(s[4], s[5], s[6], s[7]);
}

void launch_parse_be_reduce(const uint8_t *blobs, uint32_t *scalars_raw, size_t n_elems, hipStream_t st, uint32_t *zero, uint32_t zero_words,
                            uint32_t *zero2, uint32_t zero2_words) {
    unsigned grid = (unsigned)((n_elems + 255) / 256);
    prof_launch("k_parse_be_reduce", st, k_parse_be_reduce, dim3(grid), dim3(256), 0, (const uint4 *)blobs, (uint4 *)scalars_raw,
                n_elems, zero, zero_words < n_elems ? zero_words : (uint32_t)n_elems, zero2,
                zero2_words < n_elems ? zero2_words : (uint32_t)n_elems);
}

// ------------------------------------------------------------------------------------------------
// digits + counting sort

// window j of a 256-bit little-endian-limb scalar (j, and so every index below, is a compile-time
// constant after unrolling)
template <int J>
__device__ __forceinline__ uint32_t window_bits(const uint32_t *s) {
    constexpr int o = J * kWindowBits;
    constexpr int limb = o >> 5;
    constexpr int sh = o & 31;
    uint32_t v = s[limb] >> sh;
    if constexpr (sh + kWindowBits > 32 && limb + 1 < 8) v |= s[limb + 1] << (32 - sh);
    return v & ((1u << kWindowBits) - 1);
}

// calls f(j, bucket_index, negative) for every non-zero signed digit of s
template <int J, class F>
__device__ __forceinline__ void for_each_digit(const uint32_t *s, uint32_t carry, F &&f) {
    if constexpr (J < kNumWindows) {
        uint32_t raw = window_bits<J>(s) + carry;
        uint32_t neg = raw > (1u << (kWindowBits - 1)) ? 1u : 0u;
        uint32_t mag = neg ? (1u << kWindowBits) - raw : raw;  // 0 .. 2^(c-1)
        if (mag) f(J, mag - 1, neg);
        for_each_digit<J + 1>(s, neg, f);
    }
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

constexpr int kSortThreads = 1024;
constexpr int kHeavyThreshold = 64;  // buckets above this many entries get a workgroup instead of a lane
constexpr int kBucketsPerSortThread = kNumBuckets / kSortThreads;  // 4
constexpr int kScalarsPerSortThread = kBlobElems / kSortThreads;   // 4
constexpr int kStageEntries = 16384;                                // slots per pass of the scatter's LDS staging buffer (a power of two)
static_assert(kNumBuckets % kSortThreads == 0 && kBlobElems % kSortThreads == 0, "sort tiling");

// one workgroup (16 waves) per blob
template <bool staged>
__global__ __launch_bounds__(kSortThreads) void k_digit_sort(const uint4 *__restrict__ scalars,
                                                             uint32_t *__restrict__ sorted,
                                                             uint32_t *__restrict__ bucket_start,
                                                             uint32_t *__restrict__ perm) {
    __shared__ uint32_t cnt[kNumBuckets];  // histogram, then scatter cursors
    __shared__ uint32_t wave_tot[kSortThreads / 64];
    __shared__ uint32_t pop_hist[256];  // buckets per (clamped) population
    __shared__ uint32_t pop_cur[256];
    __shared__ uint32_t bst[kNumBuckets + 1];                    // bucket starts (cnt turns into the cursors)
    __shared__ uint32_t stage[kStageEntries + kHeavyThreshold];  // 64 KB + slack: one position range of the blob's entries at a time

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const size_t blob = blockIdx.x;
    const uint4 *sc = scalars + blob * (size_t)kBlobElems * 2;

    for (int k = tid; k < kNumBuckets; k += kSortThreads) cnt[k] = 0;
    if (tid < 256) pop_hist[tid] = 0;
    __syncthreads();

    // (the scalars are read twice -- for the histogram here and for the slots below -- rather than kept: 32 registers that the 80 slot
    // words need; the second read comes out of the L2)
    auto load_scalar = [&](int q, uint32_t *w) {
        const int e = q * kSortThreads + tid;
        const uint4 lo = sc[2 * e], hi = sc[2 * e + 1];
        w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
        w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
    };
#pragma unroll
    for (int q = 0; q < kScalarsPerSortThread; q++) {
        uint32_t s[8];
        load_scalar(q, s);
        for_each_digit<0>(s, 0u, [&](int, uint32_t b, uint32_t) { atomicAdd(&cnt[b], 1u); });
    }
    __syncthreads();

    // exclusive prefix sum over the 4096 bucket counts: 4 per lane, wave64 shuffle scan, 16 wave totals
    uint32_t c[kBucketsPerSortThread];
    uint32_t local = 0;
#pragma unroll
    for (int k = 0; k < kBucketsPerSortThread; k++) {
        c[k] = cnt[tid * kBucketsPerSortThread + k];
        local += c[k];
    }
    uint32_t incl = wave_inclusive_scan(local, lane);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        uint32_t t = lane < kSortThreads / 64 ? wave_tot[lane] : 0u;
        uint32_t ti = wave_inclusive_scan(t, lane);
        if (lane < kSortThreads / 64) wave_tot[lane] = ti - t;  // exclusive
    }
    __syncthreads();
    uint32_t base = wave_tot[wave] + incl - local;
    uint32_t *bs = bucket_start + blob * (size_t)(kNumBuckets + 1);
#pragma unroll
    for (int k = 0; k < kBucketsPerSortThread; k++) {
        int b = tid * kBucketsPerSortThread + k;
        bs[b] = base;
        cnt[b] = base;
        bst[b] = base;
        base += c[k];
        atomicAdd(&pop_hist[c[k] > 255u ? 255u : c[k]], 1u);
    }
    if (tid == kSortThreads - 1) {
        bs[kNumBuckets] = base;
        bst[kNumBuckets] = base;
    }
    __syncthreads();

    // order buckets by descending population so that the 64 lanes of an accumulate wave get
    // near-equal trip counts (counting sort on the clamped population)
    if (tid < 256) {
        uint32_t before = 0;
        for (int k = tid + 1; k < 256; k++) before += pop_hist[k];
        pop_cur[tid] = before;
        // buckets with more than kHeavyThreshold entries come first in the order; their number is
        // stored behind the permutation for the two accumulate kernels
        if (tid == kHeavyThreshold) perm[blob * (size_t)(kNumBuckets + 1) + kNumBuckets] = before;
    }
    __syncthreads();
    uint32_t *pm = perm + blob * (size_t)(kNumBuckets + 1);
#pragma unroll
    for (int k = 0; k < kBucketsPerSortThread; k++) {
        uint32_t pos = atomicAdd(&pop_cur[c[k] > 255u ? 255u : c[k]], 1u);
        pm[pos] = (uint32_t)(tid * kBucketsPerSortThread + k);
    }

    // scatter: entry = window * 4096 + point (the table index), sign in bit 31.
    // Each entry's slot comes from its bucket's cursor (an LDS atomic). The entries travel to global memory through an LDS staging
    // buffer, one position range of kStageEntries slots per pass, and leave it as consecutive words of consecutive lanes, i.e. as whole
    // lines. (Scattered 4-byte stores straight to `sorted` reached HBM as one 32-byte masked write each: 2.6 GB per 1024 blobs for
    // 0.34 GB of entries, and the kernel was as long as that traffic -- VERDICT r03, profiles/r02_pmc_bucket_write_size.csv.) A pass
    // takes the buckets whose FIRST slot lies in its range; a bucket of up to kHeavyThreshold entries overhangs the range by less
    // than that (the buffer's slack), a heavier one stores directly in the first pass (its slots are consecutive anyway) and its slots
    // stay marked empty in the buffer, so that the copy-out steps over them. Nothing is kept per entry
    // between the passes: every pass walks the digits again (the scalars come out of the L2).
    const uint32_t total = bst[kNumBuckets];
    uint32_t *out = sorted + blob * (size_t)kMaxEntries;
    if constexpr (!staged) {   // LWKZG_SORT_STAGE=0, the A/B arm: every entry straight to its slot (round 3's scatter)
#pragma unroll
        for (int q = 0; q < kScalarsPerSortThread; q++) {
            uint32_t s[8];
            load_scalar(q, s);
            const uint32_t e = (uint32_t)(q * kSortThreads + tid);
            for_each_digit<0>(s, 0u, [&](int j, uint32_t b, uint32_t neg) {
                out[atomicAdd(&cnt[b], 1u)] = ((uint32_t)j * kBlobElems + e) | (neg ? kEntryNegBit : 0u);
            });
        }
        return;
    }
    constexpr uint32_t kEmpty = 0xffffffffu;   // never an entry (window < 20)
    for (uint32_t p = 0; p * kStageEntries < total; p++) {
        __syncthreads();   // the previous pass's copy-out has read the buffer
        for (int k = tid; k < kStageEntries + kHeavyThreshold; k += kSortThreads) stage[k] = kEmpty;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kScalarsPerSortThread; q++) {
            uint32_t s[8];
            load_scalar(q, s);
#pragma unroll
            for (int k = 0; k < 8; k++) asm volatile("" : "+v"(s[k]));   // (this pass's own copy: hoisting the 80 digits out of the pass loop spills them)
            const uint32_t e = (uint32_t)(q * kSortThreads + tid);
            for_each_digit<0>(s, 0u, [&](int j, uint32_t b, uint32_t neg) {
                const uint32_t start = bst[b], size = bst[b + 1] - start;
                const uint32_t entry = ((uint32_t)j * kBlobElems + e) | (neg ? kEntryNegBit : 0u);
                if (size > (uint32_t)kHeavyThreshold) {
                    if (p == 0) out[atomicAdd(&cnt[b], 1u)] = entry;
                } else if (start / kStageEntries == p) {
                    stage[atomicAdd(&cnt[b], 1u) - p * kStageEntries] = entry;
                }
            });
        }
        __syncthreads();
        // the slots this pass filled leave as consecutive words of consecutive lanes; the slots of heavy buckets inside the range (written
        // directly, above) and the overhang of the previous pass's last bucket are still kEmpty here and are skipped
        for (uint32_t k = tid; k < (uint32_t)(kStageEntries + kHeavyThreshold); k += kSortThreads) {
            const uint32_t w = stage[k];
            if (w != kEmpty) out[p * kStageEntries + k] = w;
        }
    }
}

void launch_digit_sort(const uint32_t *scalars_raw, uint32_t *sorted, uint32_t *bucket_start, uint32_t *perm,
                       size_t n_blobs, hipStream_t st) {
    prof_launch("k_digit_sort", st, knobs().sort_stage ? k_digit_sort<true> : k_digit_sort<false>, dim3((unsigned)n_blobs), dim3(kSortThreads), 0,
                (const uint4 *)scalars_raw, sorted, bucket_start, perm);
}

// ------------------------------------------------------------------------------------------------
// bucket accumulation: THE hot kernel

constexpr int kAccThreads = 256;

// lane i receives lane i+d's point (all 56 limbs travel by ds_bpermute-free DPP/shuffle, no LDS)
template <class PX>
__device__ __forceinline__ PX wave_shfl_down(const PX &v, int d) {
    PX r;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        r.x.l[i] = __shfl_down(v.x.l[i], d, 64);
        r.y.l[i] = __shfl_down(v.y.l[i], d, 64);
        r.zz.l[i] = __shfl_down(v.zz.l[i], d, 64);
        r.zzz.l[i] = __shfl_down(v.zzz.l[i], d, 64);
    }
    return r;
}

// ONE launch accumulates every bucket of every blob of the batch: grid = (kHeavyBlocks + 16, blobs).
//
//  * blockIdx.x >= kHeavyBlocks -- light buckets (<= kHeavyThreshold entries; all of them for uniformly
//    random scalars): one lane per bucket, lanes ordered by population so a wave's 64 trip counts are
//    near-equal; the XYZZ accumulator never leaves VGPRs. Field products are inlined here
//    (G1Affine29i / G1Xyzz29i: no call overhead, no forced s_waitcnt at call boundaries).
//  * blockIdx.x < kHeavyBlocks -- heavy buckets: one WAVE per bucket, entries strided over the 64
//    lanes, then a shuffle tree. They are the normal case, not an edge case: blobs whose elements
//    carry 31 payload bytes (the usual EIP-4844 packing, and the bench workload) leave only the digits
//    0..2 in the top window, so ~2000 entries land in one bucket; adversarial blobs (all scalars equal)
//    put 4096 entries into each of 20 buckets. These few long-running waves are dispatched first and
//    overlap with the light blocks of the same launch.
constexpr int kHeavyBlocks = 2;                       // x 4 waves = 8 heavy buckets in flight per blob
constexpr int kLightBlocks = kNumBuckets / kAccThreads;

// heavy buckets of one blob: one WAVE per bucket, entries strided over the 64 lanes, then a shuffle tree (blocks 0 .. kHeavyBlocks - 1)
__device__ __forceinline__ void bucket_heavy_blocks(const G1Affine29 *__restrict__ table, const uint32_t *__restrict__ ent,
                                                    const uint32_t *__restrict__ bs, const uint32_t *__restrict__ pm, uint32_t n_heavy,
                                                    G1Xyzz29 *__restrict__ out, uint32_t heavy_block) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = heavy_block * (kAccThreads / 64) + (threadIdx.x >> 6);
    for (uint32_t h = wave; h < n_heavy; h += kHeavyBlocks * (kAccThreads / 64)) {
        const uint32_t b = pm[h];
        const uint32_t begin = bs[b], end = bs[b + 1];
        G1Xyzz29 acc = G1Xyzz29::infinity();
        for (uint32_t k = begin + lane; k < end; k += 64) {
            uint32_t e = ent[k];
            G1Affine29 p = table[e & ~kEntryNegBit];
            acc = xyzz_madd(acc, p.x, cneg(p.y, (e & kEntryNegBit) != 0));
        }
        for (int d = 32; d >= 1; d >>= 1) {
            G1Xyzz29 other = wave_shfl_down(acc, d);
            if (lane < d) acc = xyzz_add(acc, other);
        }
        if (lane == 0) out[b] = acc;
    }
}

// (block, blob) of this workgroup: blocks 0 .. kHeavyBlocks - 1 of a blob are its heavy blocks, the rest its light ones. (One row of
// workgroups with every blob's heavy blocks at the head of the launch was tried -- the last blobs' heavy waves would no longer start
// last -- and lost 20 %: 13.6 instead of 10.7 ms per 512-blob launch, gpurun_out r04g; the interleaved order keeps a few latency-bound
// heavy waves beside many light ones on every compute unit all the time.)
struct BucketBlock {
    size_t blob;
    uint32_t block;   // heavy: 0 .. kHeavyBlocks - 1; light: 0 .. kLightBlocks - 1
    bool heavy;
};
__device__ __forceinline__ BucketBlock bucket_block() {
    if (blockIdx.x < (uint32_t)kHeavyBlocks) return {blockIdx.y, blockIdx.x, true};
    return {blockIdx.y, blockIdx.x - kHeavyBlocks, false};
}

// one light bucket on one lane, compiler-scheduled, complete by branches (P + P, P - P, infinity): the whole light path of the A/B arm,
// and the repair of the rare lane of the hand-scheduled stream that met P = +-Q
__device__ __forceinline__ void bucket_light_lane(const G1Affine29 *__restrict__ table, const uint32_t *__restrict__ ent,
                                                  const uint32_t *__restrict__ bs, uint32_t b, G1Xyzz29 *__restrict__ out) {
    const uint32_t begin = bs[b], end = bs[b + 1];
    const G1Affine29i *tab = (const G1Affine29i *)table;
    G1Xyzz29i acc = G1Xyzz29i::infinity();
    if (begin < end) {
        // entry -> point is a dependent gather: the entry index runs two steps ahead, and the next point's gather is
        // issued inside the addition right after the current point's last use, into the registers it vacated
        // (xyzz_madd_split), with about 3k v_mad_u64_u32 of time to land
        uint32_t e = ent[begin];
        uint32_t e1 = begin + 1 < end ? ent[begin + 1] : e;
        G1Affine29i p = tab[e & ~kEntryNegBit];
        for (uint32_t k = begin; k < end; k++) {
            const auto qy = cneg(p.y, (e & kEntryNegBit) != 0);
            xyzz_madd_split(acc, p.x, qy, [&]() {
                e = e1;
                if (k + 1 < end) p = tab[e & ~kEntryNegBit];
                if (k + 2 < end) e1 = ent[k + 2];
            });
        }
    }
    ((G1Xyzz29i *)out)[b] = acc;
}

// the whole accumulation, compiler-scheduled (LWKZG_BUCKET_ASM=0: the A/B arm)
__global__ __launch_bounds__(kAccThreads) void k_bucket_accumulate(const G1Affine29 *__restrict__ table,
                                                                   const uint32_t *__restrict__ sorted,
                                                                   const uint32_t *__restrict__ bucket_start,
                                                                   const uint32_t *__restrict__ perm,
                                                                   G1Xyzz29 *__restrict__ buckets) {
    const BucketBlock bb = bucket_block();
    const size_t blob = bb.blob;
    const uint32_t *pm = perm + blob * (size_t)(kNumBuckets + 1);
    const uint32_t n_heavy = pm[kNumBuckets];
    const uint32_t *bs = bucket_start + blob * (size_t)(kNumBuckets + 1);
    const uint32_t *ent = sorted + blob * (size_t)kMaxEntries;
    G1Xyzz29 *out = buckets + blob * (size_t)kNumBuckets;
    if (bb.heavy) {
        bucket_heavy_blocks(table, ent, bs, pm, n_heavy, out, bb.block);
        return;
    }
    const uint32_t t = bb.block * kAccThreads + threadIdx.x;  // rank in the population order
    if (t < n_heavy) return;
    bucket_light_lane(table, ent, bs, pm[t], out);
}

// The light buckets as a hand-scheduled instruction stream (tools/gen_bucket_asm.py writes bucket_asm.inc and explains it): the
// mixed-addition loop of the direct-table kernel (tools/gen_direct_asm.py) fed from the lane's entry list
// instead of its scalars' digits. The heavy buckets stay with the C++ wave-per-bucket path, in the same launch (their few long
// waves are dispatched first and run beside the light blocks). The stream has no P = +-Q branches: a lane that meets one says so
// in the statement's output and its bucket is recomputed right here by the C++ formulas (never on honest data: two entries of one
// bucket would have to be the same or opposite points, or a partial sum would have to hit a table row).
__global__ __launch_bounds__(kAccThreads) void k_bucket_accumulate_asm(const G1Affine29 *__restrict__ table,
                                                                       const uint32_t *__restrict__ sorted,
                                                                       const uint32_t *__restrict__ bucket_start,
                                                                       const uint32_t *__restrict__ perm,
                                                                       G1Xyzz29 *__restrict__ buckets) {
#if defined(__HIP_DEVICE_COMPILE__)
    const BucketBlock bb = bucket_block();
    const size_t blob = bb.blob;
    const uint32_t *pm = perm + blob * (size_t)(kNumBuckets + 1);
    const uint32_t n_heavy = pm[kNumBuckets];
    const uint32_t *bs = bucket_start + blob * (size_t)(kNumBuckets + 1);
    const uint32_t *ent = sorted + blob * (size_t)kMaxEntries;
    G1Xyzz29 *out = buckets + blob * (size_t)kNumBuckets;
    if (bb.heavy) {
        bucket_heavy_blocks(table, ent, bs, pm, n_heavy, out, bb.block);
        return;
    }
    const uint32_t rank = bb.block * kAccThreads + threadIdx.x;
    uint32_t trouble;
    asm volatile(
#include "bucket_asm.inc"
        : "=&v"(trouble)
        : "s"(table), "s"(ent), "s"(bs), "s"(pm), "s"(out), "s"(n_heavy), "v"(rank)
        :
#include "bucket_asm_clobbers.inc"
    );
    if (trouble && rank >= n_heavy) bucket_light_lane(table, ent, bs, pm[rank], out);
#endif
}

static bool bucket_asm_enabled() {
    return knobs().bucket_asm;
}

void launch_bucket_accumulate(const G1Affine29 *table, const uint32_t *sorted, const uint32_t *bucket_start,
                              const uint32_t *perm, G1Xyzz29 *buckets, size_t n_blobs, hipStream_t st) {
    const dim3 grid(kHeavyBlocks + kLightBlocks, (unsigned)n_blobs);
    if (bucket_asm_enabled()) {
        prof_launch("k_bucket_accumulate_asm", st, k_bucket_accumulate_asm, grid, dim3(kAccThreads), 0, table, sorted, bucket_start, perm, buckets);
    } else {
        prof_launch("k_bucket_accumulate", st, k_bucket_accumulate, grid, dim3(kAccThreads), 0, table, sorted, bucket_start, perm, buckets);
    }
}

// ------------------------------------------------------------------------------------------------
// bucket reduction: S = sum_{k=1..NB} k * B_k per blob

// Three instantiations: 64 lanes x 64 buckets (fewest additions in total), 128 lanes x 32 buckets (large batches: half the
// chain of the former, two waves per blob) and 512 lanes x 8 buckets (shortest dependent chain: latency, small batches).

template <int kRedThreads>
__global__ __launch_bounds__(kRedThreads) void k_bucket_reduce(const G1Xyzz29 *__restrict__ buckets,
                                                               G1Xyzz29 *__restrict__ sums) {
    constexpr int kBucketsPerRedThread = kNumBuckets / kRedThreads;
    static_assert((kBucketsPerRedThread & (kBucketsPerRedThread - 1)) == 0, "chunk must be a power of two");
    __shared__ G1Xyzz29 sh[kRedThreads];
    const int t = threadIdx.x;
    const size_t blob = blockIdx.x;
    const G1Xyzz29 *B = buckets + blob * (size_t)kNumBuckets + (size_t)t * kBucketsPerRedThread;

    // lane t owns bucket values k = t*16 + 1 .. t*16 + 16:
    //   run = sum B_k,  wsum = sum (k - t*16) B_k     (descending running sums)
    G1Xyzz29 run = G1Xyzz29::infinity(), wsum = G1Xyzz29::infinity();
    for (int k = kBucketsPerRedThread - 1; k >= 0; k--) {
        run = xyzz_add(run, B[k]);
        wsum = xyzz_add(wsum, run);
    }
    // total = sum_t wsum_t + 16 * sum_t t * run_t, and sum_t t*run_t = sum_{t>=1} (suffix sum of run)_t
    sh[t] = run;
    __syncthreads();
    for (int d = 1; d < kRedThreads; d <<= 1) {
        G1Xyzz29 other = (t + d < kRedThreads) ? sh[t + d] : G1Xyzz29::infinity();
        __syncthreads();
        run = xyzz_add(run, other);
        sh[t] = run;
        __syncthreads();
    }
    // tree-sum the suffix sums over t >= 1
    sh[t] = (t >= 1) ? run : G1Xyzz29::infinity();
    __syncthreads();
    for (int d = kRedThreads / 2; d >= 1; d >>= 1) {
        if (t < d) sh[t] = xyzz_add(sh[t], sh[t + d]);
        __syncthreads();
    }
    G1Xyzz29 hi = sh[0];
    __syncthreads();
    // tree-sum the weighted sums
    sh[t] = wsum;
    __syncthreads();
    for (int d = kRedThreads / 2; d >= 1; d >>= 1) {
        if (t < d) sh[t] = xyzz_add(sh[t], sh[t + d]);
        __syncthreads();
    }
    if (t == 0) {
        for (int k = 1; k < kBucketsPerRedThread; k <<= 1) hi = xyzz_dbl(hi);
        sums[blob] = xyzz_add(sh[0], hi);
    }
}

static int reduce_lanes_override() {
    return knobs().reduce_lanes;
}

void launch_bucket_reduce(const G1Xyzz29 *buckets, G1Xyzz29 *sums, size_t n_blobs, hipStream_t st) {
    int lanes = reduce_lanes_override();
    if (lanes == 0) lanes = n_blobs <= 256 ? 512 : 128;  // r02, 1024 blobs: 2.40 ms with 128 lanes, 2.91 with 64, 3.86 with 512
    if (lanes >= 512)
        prof_launch("k_bucket_reduce", st, k_bucket_reduce<512>, dim3((unsigned)n_blobs), dim3(512), 0, buckets, sums);
    else if (lanes >= 128)
        prof_launch("k_bucket_reduce", st, k_bucket_reduce<128>, dim3((unsigned)n_blobs), dim3(128), 0, buckets, sums);
    else
        prof_launch("k_bucket_reduce", st, k_bucket_reduce<64>, dim3((unsigned)n_blobs), dim3(64), 0, buckets, sums);
}

// ------------------------------------------------------------------------------------------------
// sum of n partial results (tiled MSM: one 4096-term MSM per tile of a longer scalar vector)

constexpr int kSumThreads = 256;

__global__ __launch_bounds__(kSumThreads) void k_sum_points(const G1Xyzz29 *__restrict__ in, size_t n,
                                                            G1Xyzz29 *__restrict__ total, int accumulate) {
    __shared__ G1Xyzz29 sh[kSumThreads];
    const int t = threadIdx.x;
    G1Xyzz29 acc = G1Xyzz29::infinity();
    for (size_t i = t; i < n; i += kSumThreads) acc = xyzz_add(acc, in[i]);
    sh[t] = acc;
    __syncthreads();
    for (int d = kSumThreads / 2; d >= 1; d >>= 1) {
        if (t < d) sh[t] = xyzz_add(sh[t], sh[t + d]);
        __syncthreads();
    }
    if (t == 0) total[0] = accumulate ? xyzz_add(total[0], sh[0]) : sh[0];
}

void launch_sum_points(const G1Xyzz29 *in, size_t n, G1Xyzz29 *total, int accumulate, hipStream_t st) {
    prof_launch("k_sum_points", st, k_sum_points, dim3(1), dim3(kSumThreads), 0, in, n, total, accumulate);
}

// ------------------------------------------------------------------------------------------------
// finalize: affine + ZCash compression, one lane per result

__global__ __launch_bounds__(64) void k_finalize_compress(const G1Xyzz29 *__restrict__ sums, uint8_t *__restrict__ out48,
                                                          size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    __builtin_amdgcn_s_setprio(2);  // one inversion per lane, a pure latency chain at the end of every call (see k_direct_fold)
    uint8_t b[48];
    g1_compress(b, sums[i]);
    uint32_t *o = (uint32_t *)(out48 + 48 * i);
#pragma unroll
    for (int k = 0; k < 12; k++)
        o[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) |
               ((uint32_t)b[4 * k + 3] << 24);
}

void launch_finalize_compress(const G1Xyzz29 *sums, uint8_t *out48, size_t n, hipStream_t st) {
    prof_launch("k_finalize_compress", st, k_finalize_compress, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, sums, out48, n);
}

}  // namespace lwk
