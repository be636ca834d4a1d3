// prims_check.hip -- the primitives beneath every kernel, run one operation per case on operands given as raw limbs, for the
// HOST compile and for the DEVICE compile of the same LWK_HD sources (tests/test_prims_cpu.py, tests/test_gpu_prims.py; the cases and
// the big-integer expectations are tests/prims_cases.py). The device build is where operator* / sqr are calls or inlined bodies, where
// mul_sub<INL = true> is the fused mont_mul_add29 over neg(c), where fe_mul is fe_mul_call, and where the G1Xyzz29i instantiations
// of the group law exist at all.
//
//   prims_check host|device <cases-file> <results-file>
//   case line:    <op> <instantiation> <hex words of the operands, the internal representation (limbs), in order>
//   result line:  <hex words the operation returned>; a field element is its 14 limbs, then BOUND and LIMB of the returned TYPE
//
// device mode: one kernel per family, one case per lane, a lane writes its own result slot only; one launch set, then exit.
//   for F in A B C D Di E: hipcc -DLWK_LIMB_BITS=28 -O3 -std=c++17 --offload-arch=gfx950 -I lambdaworks_kzg_amd/csrc -DPC_FAM=F -c ...
//   once more without -DPC_FAM (main), then link the seven objects with hipcc (prims_cases.py: build_checker)
//   (host mode only: add --cuda-host-only -DPRIMS_HOST_ONLY, which leaves the kernels out)
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "g1.cuh"
#include "fr28.cuh"
#include "glv.cuh"
using namespace lwk;

#define PC_IN 112   // words of a case's operands (two XYZZ points)
#define PC_OUT 64   // words of a case's result slot: [0] = count, then the words
#define PC_OP __host__ __device__ __noinline__ static void
#define PC_HD __host__ __device__ __forceinline__

template <class F>
PC_HD F ld(const uint32_t *in) {
    F r;
    for (int i = 0; i < 14; i++) r.l[i] = in[i];
    return r;
}
template <class F>
PC_HD void st(uint32_t *out, const F &r) {
    out[0] = 16;
    for (int i = 0; i < 14; i++) out[1 + i] = r.l[i];
    out[15] = (uint32_t)F::BOUND;
    out[16] = (uint32_t)F::LIMB;
}
PC_HD void st_words(uint32_t *out, const uint32_t *w, int n) {
    out[0] = (uint32_t)n;
    for (int i = 0; i < n; i++) out[1 + i] = w[i];
}
PC_HD void st_flag(uint32_t *out, bool f) {
    out[0] = 1;
    out[1] = f ? 1u : 0u;
}

// ---- A. products ------------------------------------------------------------------------------------------------------------
template <int A, int LA, int B, int LB, bool I>
PC_OP op_mul(const uint32_t *in, uint32_t *out) {
    st(out, ld<F29<A, I, LA>>(in) * ld<F29<B, I, LB>>(in + 14));
}
template <int A, int LA, bool I>
PC_OP op_sqr(const uint32_t *in, uint32_t *out) {
    st(out, sqr(ld<F29<A, I, LA>>(in)));
}
template <int A, int LA, int B, int LB, int C, int LC, int D, int LD, bool I>
PC_OP op_mul_sub(const uint32_t *in, uint32_t *out) {
    st(out, mul_sub(ld<F29<A, I, LA>>(in), ld<F29<B, I, LB>>(in + 14), ld<F29<C, I, LC>>(in + 28), ld<F29<D, I, LD>>(in + 42)));
}

#define PC_MUL(X, A, LA, B, LB)                                            \
    X("mul", #A "," #LA "," #B "," #LB ",0", (op_mul<A, LA, B, LB, false>)) \
    X("mul", #A "," #LA "," #B "," #LB ",1", (op_mul<A, LA, B, LB, true>))
#define PC_SQR(X, A, LA)                                 \
    X("sqr", #A "," #LA ",0", (op_sqr<A, LA, false>))     \
    X("sqr", #A "," #LA ",1", (op_sqr<A, LA, true>))
#define PC_MULSUB(X, A, LA, B, LB, C, LC, D, LD)                                                                        \
    X("mul_sub", #A "," #LA "," #B "," #LB "," #C "," #LC "," #D "," #LD ",0", (op_mul_sub<A, LA, B, LB, C, LC, D, LD, false>)) \
    X("mul_sub", #A "," #LA "," #B "," #LB "," #C "," #LC "," #D "," #LD ",1", (op_mul_sub<A, LA, B, LB, C, LC, D, LD, true>))
// the last three mul_sub rows are the ones xyzz_madd, xyzz_add / xyzz_dbl_affine and xyzz_dbl make
#define FAM_A(X)                                                                                                              \
    PC_MUL(X, 2, 1, 2, 1) PC_MUL(X, 14, 1, 6, 1) PC_MUL(X, 2048, 1, 1, 1) PC_MUL(X, 1, 14, 1, 1) PC_MUL(X, 32, 4, 64, 4)       \
    PC_MUL(X, 2, 4, 1024, 4) PC_MUL(X, 128, 2, 16, 8) PC_MUL(X, 45, 1, 45, 1)                                                  \
    PC_SQR(X, 2, 1) PC_SQR(X, 45, 4) PC_SQR(X, 32, 3) PC_SQR(X, 14, 2)                                                         \
    PC_MULSUB(X, 2, 1, 2, 1, 6, 1, 2, 1) PC_MULSUB(X, 32, 2, 32, 4, 15, 3, 64, 1) PC_MULSUB(X, 2, 1, 30, 8, 6, 1, 2, 1)        \
    PC_MULSUB(X, 1, 1, 1, 1, 31, 7, 63, 1)                                                                                     \
    PC_MULSUB(X, 10, 3, 18, 3, 6, 1, 2, 1) PC_MULSUB(X, 6, 3, 18, 3, 2, 1, 2, 1) PC_MULSUB(X, 6, 3, 18, 3, 2, 1, 6, 1)

// ---- B. sums and tests ------------------------------------------------------------------------------------------------------
template <int A, int LA, int B, int LB>
PC_OP op_add(const uint32_t *in, uint32_t *out) {
    st(out, ld<F29<A, false, LA>>(in) + ld<F29<B, false, LB>>(in + 14));
}
template <int A, int LA, int B, int LB>
PC_OP op_sub(const uint32_t *in, uint32_t *out) {
    st(out, ld<F29<A, false, LA>>(in) - ld<F29<B, false, LB>>(in + 14));
}
template <int A, int LA, int B, int LB>
PC_OP op_sub_is_zero(const uint32_t *in, uint32_t *out) {
    st_flag(out, (ld<F29<A, false, LA>>(in) - ld<F29<B, false, LB>>(in + 14)).is_zero());
}
template <int A, int LA>
PC_OP op_dbl(const uint32_t *in, uint32_t *out) {
    st(out, dbl(ld<F29<A, false, LA>>(in)));
}
template <int A, int LA>
PC_OP op_neg(const uint32_t *in, uint32_t *out) {
    st(out, neg(ld<F29<A, false, LA>>(in)));
}
template <int A, int LA>
PC_OP op_cneg(const uint32_t *in, uint32_t *out) {
    st(out, cneg(ld<F29<A, false, LA>>(in), in[14] != 0));
}
template <int A, int LA>
PC_OP op_normed(const uint32_t *in, uint32_t *out) {
    st(out, normed(ld<F29<A, false, LA>>(in)));
}
template <int A, int LA>
PC_OP op_is_zero(const uint32_t *in, uint32_t *out) {
    st_flag(out, ld<F29<A, false, LA>>(in).is_zero());
}
template <int A, int LA>
PC_OP op_is_literal_zero(const uint32_t *in, uint32_t *out) {
    st_flag(out, ld<F29<A, false, LA>>(in).is_literal_zero());
}

#define PC_BIN(X, A, LA, B, LB)                                            \
    X("add", #A "," #LA "," #B "," #LB, (op_add<A, LA, B, LB>))             \
    X("sub", #A "," #LA "," #B "," #LB, (op_sub<A, LA, B, LB>))             \
    X("sub_is_zero", #A "," #LA "," #B "," #LB, (op_sub_is_zero<A, LA, B, LB>))
#define PC_UN(X, A, LA)                                           \
    X("dbl", #A "," #LA, (op_dbl<A, LA>))                          \
    X("neg", #A "," #LA, (op_neg<A, LA>))                          \
    X("cneg", #A "," #LA, (op_cneg<A, LA>))                        \
    X("normed", #A "," #LA, (op_normed<A, LA>))                    \
    X("is_zero", #A "," #LA, (op_is_zero<A, LA>))                  \
    X("is_literal_zero", #A "," #LA, (op_is_literal_zero<A, LA>))
// the second PC_BIN row holds the differences the group law's formulas make; PC_UN: every operand type of the first row
#define FAM_B(X)                                                                                                           \
    PC_BIN(X, 2, 1, 2, 1) PC_BIN(X, 2, 1, 14, 3) PC_BIN(X, 14, 5, 6, 7) PC_BIN(X, 2, 1, 31, 7) PC_BIN(X, 6, 2, 3, 2)        \
    PC_BIN(X, 1, 1, 15, 1)                                                                                                  \
    PC_BIN(X, 2, 1, 14, 1) PC_BIN(X, 2, 1, 6, 1) PC_BIN(X, 6, 3, 4, 2) PC_BIN(X, 2, 1, 4, 2) PC_BIN(X, 2, 1, 10, 1)         \
    PC_UN(X, 2, 1) PC_UN(X, 14, 3) PC_UN(X, 14, 5) PC_UN(X, 6, 7) PC_UN(X, 31, 7) PC_UN(X, 6, 2) PC_UN(X, 3, 2)             \
    PC_UN(X, 1, 1) PC_UN(X, 15, 1)

// ---- C. conversions ---------------------------------------------------------------------------------------------------------
PC_OP op_from_raw(const uint32_t *in, uint32_t *out) { st(out, f29_from_raw32(in)); }
// to_raw(from_raw(raw)): raw mod p, for any raw < 2^384
PC_OP op_raw_roundtrip(const uint32_t *in, uint32_t *out) {
    uint32_t raw[12];
    f29_to_raw32(raw, f29_from_raw32(in));
    st_words(out, raw, 12);
}
template <int A, int LA>
PC_OP op_to_raw(const uint32_t *in, uint32_t *out) {
    uint32_t raw[12];
    f29_to_raw32(raw, ld<F29<A, false, LA>>(in));
    st_words(out, raw, 12);
}
template <int A, int LA>
PC_OP op_inv(const uint32_t *in, uint32_t *out) {
    st(out, f29_inv(ld<F29<A, false, LA>>(in)));
}
template <int A, int LA>
PC_OP op_inv_fermat(const uint32_t *in, uint32_t *out) {
    st(out, f29_inv_fermat(ld<F29<A, false, LA>>(in)));
}
// a^((p + 1) / 4), the exponent of the square root (g1.cuh)
template <int A, int LA>
PC_OP op_pow_sqrt(const uint32_t *in, uint32_t *out) {
    const uint32_t e[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                            0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
    st(out, f29_pow<12>(ld<F29<A, false, LA>>(in), e));
}
#define PC_CONV(X, A, LA)                                   \
    X("to_raw", #A "," #LA, (op_to_raw<A, LA>))              \
    X("inv", #A "," #LA, (op_inv<A, LA>))                    \
    X("inv_fermat", #A "," #LA, (op_inv_fermat<A, LA>))      \
    X("pow_sqrt", #A "," #LA, (op_pow_sqrt<A, LA>))
#define FAM_C(X)                                                                                   \
    X("from_raw", "-", (op_from_raw)) X("raw_roundtrip", "-", (op_raw_roundtrip)) PC_CONV(X, 2, 1) \
    PC_CONV(X, 14, 3) PC_CONV(X, 2048, 1) PC_CONV(X, 45, 14)

// ---- D. group law -----------------------------------------------------------------------------------------------------------
template <bool I>
struct Pt {
    typedef XyzzT<F29<14, I>, F29<6, I>, F29<2, I>> X;
};
template <bool I>
PC_HD typename Pt<I>::X ld_xyzz(const uint32_t *in) {
    typename Pt<I>::X r;
    r.x = ld<F29<14, I>>(in);
    r.y = ld<F29<6, I>>(in + 14);
    r.zz = ld<F29<2, I>>(in + 28);
    r.zzz = ld<F29<2, I>>(in + 42);
    return r;
}
template <class X>
PC_HD void st_xyzz(uint32_t *out, const X &r) {
    out[0] = 56;
    for (int i = 0; i < 14; i++) {
        out[1 + i] = r.x.l[i];
        out[15 + i] = r.y.l[i];
        out[29 + i] = r.zz.l[i];
        out[43 + i] = r.zzz.l[i];
    }
}
template <bool I>
PC_OP op_madd(const uint32_t *in, uint32_t *out) {
    st_xyzz(out, xyzz_madd(ld_xyzz<I>(in), ld<F29<2, I>>(in + 56), ld<F29<2, I>>(in + 70)));
}
template <bool I>
PC_OP op_madd_split(const uint32_t *in, uint32_t *out) {
    auto acc = ld_xyzz<I>(in);
    xyzz_madd_split(acc, ld<F29<2, I>>(in + 56), ld<F29<2, I>>(in + 70), [] {});
    st_xyzz(out, acc);
}
template <bool I>
PC_OP op_xadd(const uint32_t *in, uint32_t *out) {
    st_xyzz(out, xyzz_add(ld_xyzz<I>(in), ld_xyzz<I>(in + 56)));
}
template <bool I>
PC_OP op_xdbl(const uint32_t *in, uint32_t *out) {
    st_xyzz(out, xyzz_dbl(ld_xyzz<I>(in)));
}
template <bool I>
PC_OP op_xdbl_affine(const uint32_t *in, uint32_t *out) {
    st_xyzz(out, xyzz_dbl_affine<typename Pt<I>::X>(ld<F29<2, I>>(in), ld<F29<2, I>>(in + 14)));
}
// two tables, Di the inlined flavour: the group law is the long compile, so each flavour gets its own translation unit
#define PC_G(X, I, INL)                                                                                                    \
    X("xyzz_madd", I, (op_madd<INL>)) X("xyzz_madd_split", I, (op_madd_split<INL>)) X("xyzz_add", I, (op_xadd<INL>))        \
    X("xyzz_dbl", I, (op_xdbl<INL>)) X("xyzz_dbl_affine", I, (op_xdbl_affine<INL>))
#define FAM_D(X) PC_G(X, "0", false)
#define FAM_Di(X) PC_G(X, "1", true)

// ---- E. scalar side ---------------------------------------------------------------------------------------------------------
PC_HD Fr28 ld28(const uint32_t *in) {
    Fr28 r;
    for (int i = 0; i < 10; i++) r.l[i] = in[i];
    return r;
}
template <class P>
PC_HD Fe<P> ldfe(const uint32_t *in) {
    Fe<P> r;
    for (int i = 0; i < P::N; i++) r.l[i] = in[i];
    return r;
}
PC_OP op_fr28_mul(const uint32_t *in, uint32_t *out) { st_words(out, fr28_mul(ld28(in), ld28(in + 10)).l, 10); }
PC_OP op_fr28_add(const uint32_t *in, uint32_t *out) { st_words(out, fr28_add(ld28(in), ld28(in + 10)).l, 10); }
PC_OP op_fr28_sub(const uint32_t *in, uint32_t *out) { st_words(out, fr28_sub(ld28(in), ld28(in + 10)).l, 10); }
PC_OP op_fr28_norm(const uint32_t *in, uint32_t *out) { st_words(out, fr28_norm(ld28(in)).l, 10); }
PC_OP op_fr28_canonical(const uint32_t *in, uint32_t *out) { st_words(out, fr28_canonical(ld28(in)).l, 10); }
PC_OP op_fr28_to_raw_scaled(const uint32_t *in, uint32_t *out) {
    uint32_t w[8];
    fr28_to_raw_scaled(w, ld28(in));
    st_words(out, w, 8);
}
PC_OP op_fr28_from_mont256(const uint32_t *in, uint32_t *out) { st_words(out, fr28_from_mont256(ldfe<FrParams>(in)).l, 10); }
PC_OP op_fr28_to_mont256(const uint32_t *in, uint32_t *out) { st_words(out, fr28_to_mont256(ld28(in)).l, 8); }
#define PC_F28C(NAME) \
    PC_OP op_fr28_mul_const_##NAME(const uint32_t *in, uint32_t *out) { st_words(out, LWK_FR28_MUL_CONST(ld28(in), NAME).l, 10); }
PC_F28C(TO28) PC_F28C(NINV_RAW) PC_F28C(TO256) PC_F28C(RR) PC_F28C(ONE) PC_F28C(R3) PC_F28C(NINV_M)

template <class P> PC_OP op_fe_mul(const uint32_t *in, uint32_t *out) { st_words(out, fe_mul<P>(ldfe<P>(in), ldfe<P>(in + P::N)).l, P::N); }
template <class P> PC_OP op_fe_add(const uint32_t *in, uint32_t *out) { st_words(out, fe_add<P>(ldfe<P>(in), ldfe<P>(in + P::N)).l, P::N); }
template <class P> PC_OP op_fe_sub(const uint32_t *in, uint32_t *out) { st_words(out, fe_sub<P>(ldfe<P>(in), ldfe<P>(in + P::N)).l, P::N); }
template <class P> PC_OP op_fe_neg(const uint32_t *in, uint32_t *out) { st_words(out, neg(ldfe<P>(in)).l, P::N); }
template <class P> PC_OP op_fe_sqr(const uint32_t *in, uint32_t *out) { st_words(out, sqr(ldfe<P>(in)).l, P::N); }
template <class P> PC_OP op_fe_inv(const uint32_t *in, uint32_t *out) { st_words(out, inv(ldfe<P>(in)).l, P::N); }
PC_OP op_fp_inv_fermat(const uint32_t *in, uint32_t *out) { st_words(out, inv_fermat(ldfe<FpParams>(in)).l, 12); }
PC_OP op_fr_inv_divsteps(const uint32_t *in, uint32_t *out) { st_words(out, inv_divsteps(ldfe<FrParams>(in)).l, 8); }
PC_OP op_split(const uint32_t *in, uint32_t *out) {
    uint32_t w[8];
    split_by_z2(w, w + 4, in);
    st_words(out, w, 8);
}
PC_OP op_split_barrett(const uint32_t *in, uint32_t *out) {
    uint32_t w[8];
    split_by_z2_barrett(w, w + 4, in);
    st_words(out, w, 8);
}
#define PC_FE(X, NAME, P)                                                                                         \
    X(NAME "_mul", "-", (op_fe_mul<P>)) X(NAME "_add", "-", (op_fe_add<P>)) X(NAME "_sub", "-", (op_fe_sub<P>))    \
    X(NAME "_neg", "-", (op_fe_neg<P>)) X(NAME "_sqr", "-", (op_fe_sqr<P>)) X(NAME "_inv", "-", (op_fe_inv<P>))
#define FAM_E(X)                                                                                                          \
    X("fr28_mul", "-", (op_fr28_mul)) X("fr28_add", "-", (op_fr28_add)) X("fr28_sub", "-", (op_fr28_sub))                  \
    X("fr28_norm", "-", (op_fr28_norm)) X("fr28_canonical", "-", (op_fr28_canonical))                                     \
    X("fr28_to_raw_scaled", "-", (op_fr28_to_raw_scaled)) X("fr28_from_mont256", "-", (op_fr28_from_mont256))             \
    X("fr28_to_mont256", "-", (op_fr28_to_mont256))                                                                       \
    X("fr28_mul_const", "TO28", (op_fr28_mul_const_TO28)) X("fr28_mul_const", "NINV_RAW", (op_fr28_mul_const_NINV_RAW))   \
    X("fr28_mul_const", "TO256", (op_fr28_mul_const_TO256)) X("fr28_mul_const", "RR", (op_fr28_mul_const_RR))             \
    X("fr28_mul_const", "ONE", (op_fr28_mul_const_ONE)) X("fr28_mul_const", "R3", (op_fr28_mul_const_R3))                 \
    X("fr28_mul_const", "NINV_M", (op_fr28_mul_const_NINV_M))                                                             \
    PC_FE(X, "fp", FpParams) PC_FE(X, "fr", FrParams)                                                                     \
    X("fp_inv_fermat", "-", (op_fp_inv_fermat)) X("fr_inv_divsteps", "-", (op_fr_inv_divsteps))                           \
    X("split_by_z2", "-", (op_split)) X("split_by_z2_barrett", "-", (op_split_barrett))

// ---- the tables: one translation unit per family (-DPC_FAM=A, B, C, D, Di or E: its names, a dispatcher, a kernel, its launch), and
// one without PC_FAM that holds main() -- seven compiles side by side instead of one long one
struct FamilyApi {
    const char *const *names;
    int n_names;
    void (*run)(int, const uint32_t *, uint32_t *);                        // host compile
    void (*launch)(const int *, const uint32_t *, uint32_t *, int);        // device compile; null in a host-only build
};
#define X_NAME(op, inst, fn) op " " inst,
#define X_RUN(op, inst, fn)  \
    if (id == k) {           \
        fn(in, out);         \
        return;              \
    }                        \
    k++;
#if defined(PRIMS_HOST_ONLY)
#define PC_DEVICE_SIDE(F) static constexpr void (*launch_##F)(const int *, const uint32_t *, uint32_t *, int) = nullptr;
#else
#define PC_DEVICE_SIDE(F)                                                                                              \
    __global__ void __launch_bounds__(64) k_family_##F(const int *ids, const uint32_t *in, uint32_t *out, int n) {     \
        const int lane = blockIdx.x * blockDim.x + threadIdx.x;                                                        \
        if (lane >= n) return;                                                                                         \
        run_##F(ids[lane], in + (size_t)lane * PC_IN, out + (size_t)lane * PC_OUT);                                    \
    }                                                                                                                  \
    static void launch_##F(const int *ids, const uint32_t *in, uint32_t *out, int n) {                                 \
        k_family_##F<<<dim3((n + 63) / 64), dim3(64)>>>(ids, in, out, n);                                              \
    }
#endif
#define PC_FAMILY(F)                                                                                                   \
    static const char *const names_##F[] = {FAM_##F(X_NAME)};                                                          \
    __host__ __device__ static void run_##F(int id, const uint32_t *in, uint32_t *out) {                               \
        int k = 0;                                                                                                     \
        FAM_##F(X_RUN)(void) k;                                                                                        \
    }                                                                                                                  \
    PC_DEVICE_SIDE(F)                                                                                                  \
    FamilyApi pc_family_##F() { return {names_##F, (int)(sizeof(names_##F) / sizeof(names_##F[0])), run_##F, launch_##F}; }
#define PC_FAMILY_OF(F) PC_FAMILY(F)

#if defined(PC_FAM)
PC_FAMILY_OF(PC_FAM)
#else
FamilyApi pc_family_A();
FamilyApi pc_family_B();
FamilyApi pc_family_C();
FamilyApi pc_family_D();
FamilyApi pc_family_Di();
FamilyApi pc_family_E();

struct Family {
    FamilyApi api;
    std::vector<int> ids;             // per case: the row of the family's table
    std::vector<uint32_t> in, out;
};

#define HIP_OK(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "prims_check: %s failed: %s\n", #call, hipGetErrorString(e_)); \
            exit(3);                                                                      \
        }                                                                                 \
    } while (0)

static void run_on_device(Family &f) {
    const int n = (int)f.ids.size();
    int *d_ids;
    uint32_t *d_in, *d_out;
    HIP_OK(hipMalloc(&d_ids, n * sizeof(int)));
    HIP_OK(hipMalloc(&d_in, f.in.size() * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&d_out, f.out.size() * sizeof(uint32_t)));
    HIP_OK(hipMemcpy(d_ids, f.ids.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_in, f.in.data(), f.in.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0, f.out.size() * sizeof(uint32_t)));
    if (!f.api.launch) {
        fprintf(stderr, "prims_check: built without device code\n");
        exit(2);
    }
    f.api.launch(d_ids, d_in, d_out, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(f.out.data(), d_out, f.out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_ids));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
}

int main(int argc, char **argv) {
    if (argc != 4 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) {
        fprintf(stderr, "usage: prims_check host|device <cases-file> <results-file>\n");
        return 2;
    }
    const bool device = !strcmp(argv[1], "device");
    const int kFamilies = 6;
    Family fams[kFamilies];
    fams[0].api = pc_family_A();
    fams[1].api = pc_family_B();
    fams[2].api = pc_family_C();
    fams[3].api = pc_family_D();
    fams[4].api = pc_family_E();
    fams[5].api = pc_family_Di();
    FILE *fi = fopen(argv[2], "r");
    if (!fi) {
        fprintf(stderr, "prims_check: cannot read %s\n", argv[2]);
        return 2;
    }
    std::vector<std::pair<int, int>> where;  // per line: family, index in it
    std::vector<char> buf(1 << 16);
    while (fgets(buf.data(), (int)buf.size(), fi)) {
        char *save = nullptr;
        const char *op = strtok_r(buf.data(), " \n", &save), *inst = strtok_r(nullptr, " \n", &save);
        if (!op || !inst) {
            fprintf(stderr, "prims_check: line %zu: no op or instantiation\n", where.size() + 1);
            return 2;
        }
        const std::string key = std::string(op) + " " + inst;
        int fam = -1, id = -1;
        for (int f = 0; f < kFamilies && fam < 0; f++)
            for (int k = 0; k < fams[f].api.n_names; k++)
                if (key == fams[f].api.names[k]) {
                    fam = f;
                    id = k;
                    break;
                }
        if (fam < 0) {
            fprintf(stderr, "prims_check: line %zu: no instantiation '%s'\n", where.size() + 1, key.c_str());
            return 2;
        }
        Family &f = fams[fam];
        const size_t base = f.in.size();
        f.in.resize(base + PC_IN, 0u);
        int nw = 0;
        for (const char *t; (t = strtok_r(nullptr, " \n", &save));) {
            if (nw >= PC_IN) {
                fprintf(stderr, "prims_check: line %zu: more than %d words\n", where.size() + 1, PC_IN);
                return 2;
            }
            f.in[base + nw++] = (uint32_t)strtoul(t, nullptr, 16);
        }
        where.push_back({fam, (int)f.ids.size()});
        f.ids.push_back(id);
    }
    fclose(fi);
    for (Family &f : fams) {
        const int n = (int)f.ids.size();
        if (!n) continue;
        f.out.assign((size_t)n * PC_OUT, 0u);
        if (device) {
            run_on_device(f);
        } else {
            for (int i = 0; i < n; i++) f.api.run(f.ids[i], f.in.data() + (size_t)i * PC_IN, f.out.data() + (size_t)i * PC_OUT);
        }
    }
    FILE *fo = fopen(argv[3], "w");
    if (!fo) {
        fprintf(stderr, "prims_check: cannot write %s\n", argv[3]);
        return 2;
    }
    for (const auto &w : where) {
        const uint32_t *o = fams[w.first].out.data() + (size_t)w.second * PC_OUT;
        if (o[0] == 0 || o[0] >= PC_OUT) {
            fprintf(stderr, "prims_check: a case returned %u words\n", o[0]);
            return 4;
        }
        for (uint32_t i = 0; i < o[0]; i++) fprintf(fo, i ? " %x" : "%x", o[1 + i]);
        fputc('\n', fo);
    }
    if (fclose(fo)) return 2;
    return 0;
}
#endif  // PC_FAM
