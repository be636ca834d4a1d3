"""Cases and big-integer expectations for tests/prims_check.hip (tests/test_prims_cpu.py: the host compile, tests/test_gpu_prims.py: the
device compile). Plain Python integers, seeded, exact: no tolerances anywhere.

A case is one line `<op> <instantiation> <hex words>`: the operands in the INTERNAL representation (14 limbs of 28 bits for the lazy
field, 10 for fr28, 12 / 8 words for the CIOS fields), so that limbs at the top of their lazy range -- which honest data reaches with
probability 2^-28 per limb -- can be injected. Every operand satisfies the documented precondition of its slot: value < B p, limbs
0..12 < LB 2^28 for a slot of type F29<B, INL, LB>. The operand generators of a slot:
  zero        the literal zero
  saturated   limbs 0..12 all LB 2^28 - 1, the top limb the largest that keeps the value < B p
  random lazy a random value < B p in a random lazy decomposition (carries pushed back down, limbs anywhere below LB 2^28)
  k p         a multiple of the modulus, normalised or lazily decomposed
"""
import itertools
import os
import random
import shutil
import subprocess
import time

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
W = 28
MASK = (1 << W) - 1
RADIX = 1 << (14 * W)            # the lazy field's Montgomery radix
RINV = pow(RADIX, -1, P)
RADIX28 = 1 << 280               # fr28's
Z2 = 0xac45a4010001a4020000000100000000
SQRT_E = (P + 1) // 4
GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1
assert (GY * GY - GX * GX * GX - 4) % P == 0

FAMILIES = ("products", "sums", "conversions", "group", "scalar")


# ---- field29.cuh's type arithmetic, restated ---------------------------------------------------------------------------------
def sub_offset(b):
    return 2 if b < 2 else 4 if b < 4 else 8 if b < 8 else 16 if b < 16 else 32


def sub_borrow(lb):
    return 1 if lb <= 1 else 4 if lb + 1 <= 4 else 8


# ---- limbs -------------------------------------------------------------------------------------------------------------------
def val(limbs, w=W):
    return sum(l << (w * i) for i, l in enumerate(limbs))


def normal(v, n=14):
    out = [(v >> (W * i)) & MASK for i in range(n - 1)] + [v >> (W * (n - 1))]
    assert out[-1] < 1 << 32
    return out


def lazify(limbs, lb, rnd):
    """the same integer with carries pushed back down: limbs 0..n-2 land anywhere below lb 2^28"""
    l = list(limbs)
    for i in range(len(l) - 1, 0, -1):
        t = rnd.randint(0, min(l[i], lb - 1))
        l[i] -= t
        l[i - 1] += t << W
    assert val(l) == val(limbs) and all(x < lb << W for x in l[:-1]) and l[-1] < 1 << 32
    return l


def lazy(v, lb, rnd, n=14):
    return lazify(normal(v, n), lb, rnd)


def saturated(b, lb, mod=P, n=14):
    low = [(lb << W) - 1] * (n - 1)
    top = (b * mod - 1 - val(low)) >> (W * (n - 1))
    assert 0 <= top < 1 << 32, (b, lb)
    return low + [top]


def words(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def slot_operands(b, lb, rnd, mod=P, n=14):
    """the four generators for a slot of type (b, lb); the multiples of the modulus here are (b - 1) p lazily and p (or 0) normalised"""
    return {
        "zero": [0] * n,
        "sat": saturated(b, lb, mod, n),
        "rnd": lazy(rnd.randrange(b * mod), lb, rnd, n),
        "kp": lazy((b - 1) * mod, lb, rnd, n),
        "p": normal(min(1, b - 1) * mod, n),
    }


class Case:
    def __init__(self, family, op, inst, operand_words, check, note=""):
        self.family, self.op, self.inst, self.check, self.note = family, op, inst, check, note
        assert all(0 <= w < 1 << 32 for w in operand_words)
        self.line = "%s %s %s" % (op, inst, " ".join("%x" % w for w in operand_words))

    def __repr__(self):
        return "%s %s %s" % (self.op, self.inst, self.note)


def check_elem(out, want, bound=None, limb=None, allow_equal=False, mod=P):
    """a returned field element: 14 limbs, then BOUND and LIMB of the returned type. value = want (mod p), value < BOUND p (<= where
    allow_equal), limbs 0..12 < LIMB 2^28; bound / limb: what the returned type must declare"""
    assert len(out) == 16, len(out)
    limbs, got_bound, got_limb = out[:14], out[14], out[15]
    if bound is not None:
        assert got_bound in (bound if isinstance(bound, tuple) else (bound,)), ("declared bound", got_bound, bound)
    if limb is not None:
        assert got_limb == limb, ("declared limb bound", got_limb, limb)
    v = val(limbs)
    assert v % mod == want % mod, "value differs mod p"
    assert v <= got_bound * mod if allow_equal else v < got_bound * mod, ("value bound", got_bound, v // mod)
    assert all(l < got_limb << W for l in limbs[:13]), ("limb bound", got_limb)


# ---- A. products ---------------------------------------------------------------------------------------------------------------
MUL_INSTS = [(2, 1, 2, 1), (14, 1, 6, 1), (2048, 1, 1, 1), (1, 14, 1, 1), (32, 4, 64, 4), (2, 4, 1024, 4), (128, 2, 16, 8), (45, 1, 45, 1)]
SQR_INSTS = [(2, 1), (45, 4), (32, 3), (14, 2)]
# the last three are the ones xyzz_madd, xyzz_add / xyzz_dbl_affine and xyzz_dbl make
MULSUB_INSTS = [(2, 1, 2, 1, 6, 1, 2, 1), (32, 2, 32, 4, 15, 3, 64, 1), (2, 1, 30, 8, 6, 1, 2, 1), (1, 1, 1, 1, 31, 7, 63, 1),
                (10, 3, 18, 3, 6, 1, 2, 1), (6, 3, 18, 3, 2, 1, 2, 1), (6, 3, 18, 3, 2, 1, 6, 1)]


def _inst(t, inl=None):
    return ",".join(str(x) for x in t) + ("" if inl is None else ",%d" % inl)


def products(rnd, mode):
    cases = []
    for inst in MUL_INSTS:
        a_, la, b_, lb = inst
        for inl in (0, 1):
            oa, ob = slot_operands(a_, la, rnd), slot_operands(b_, lb, rnd)
            pairs = [(oa[x], ob[y], x + "*" + y) for x in oa for y in ob]
            pairs.append((lazy(rnd.randrange(a_ * P), la, rnd), lazy(rnd.randrange(b_ * P), lb, rnd), "rnd*rnd"))
            for a, b, note in pairs:
                want = val(a) * val(b) * RINV
                cases.append(Case("products", "mul", _inst(inst, inl), a + b,
                                  lambda out, want=want: check_elem(out, want, bound=2, limb=1), note))
    for inst in SQR_INSTS:
        a_, la = inst
        for inl in (0, 1):
            oa = slot_operands(a_, la, rnd)
            ops = list(oa.items()) + [("rnd", lazy(rnd.randrange(a_ * P), la, rnd)) for _ in range(5)]
            for note, a in ops:
                want = val(a) * val(a) * RINV
                cases.append(Case("products", "sqr", _inst(inst, inl), a,
                                  lambda out, want=want: check_elem(out, want, bound=2, limb=1), note))
    for inst in MULSUB_INSTS:
        slots = [(inst[0], inst[1]), (inst[2], inst[3]), (inst[4], inst[5]), (inst[6], inst[7])]
        for inl in (0, 1):
            # the inlined flavour of the DEVICE compile is the fused product pair (< 2p); everything else is two products and a
            # subtraction (< 6p). The two need not agree limb for limb.
            bound = 2 if (inl and mode == "device") else 6
            def gen(kind, slot):
                b, lb = slot
                return slot_operands(b, lb, rnd)[kind]
            picks = [list(t) for t in itertools.product(("sat", "rnd"), repeat=4)]
            for i in range(4):
                picks.append(["zero" if j == i else "sat" for j in range(4)])
                picks.append(["kp" if j == i else "rnd" for j in range(4)])
            picks += [["zero"] * 4, ["kp"] * 4, ["p", "sat", "p", "sat"]] + [["rnd"] * 4] * 3
            for pick in picks:
                a, b, c, d = (gen(k, s) for k, s in zip(pick, slots))
                want = (val(a) * val(b) - val(c) * val(d)) * RINV
                cases.append(Case("products", "mul_sub", _inst(inst, inl), a + b + c + d,
                                  lambda out, want=want, bound=bound: check_elem(out, want, bound=bound, limb=1), ",".join(pick)))
    return cases


# ---- B. sums and tests -----------------------------------------------------------------------------------------------------------
# the second row: the differences the group law's formulas make
BIN_INSTS = [(2, 1, 2, 1), (2, 1, 14, 3), (14, 5, 6, 7), (2, 1, 31, 7), (6, 2, 3, 2), (1, 1, 15, 1),
             (2, 1, 14, 1), (2, 1, 6, 1), (6, 3, 4, 2), (2, 1, 4, 2), (2, 1, 10, 1)]
UN_INSTS = [(2, 1), (14, 3), (14, 5), (6, 7), (31, 7), (6, 2), (3, 2), (1, 1), (15, 1)]


def _flag(want):
    def check(out):
        assert out == [int(want)], (out, want)
    return check


def sums(rnd, mode):
    cases = []
    for inst in BIN_INSTS:
        a_, la, b_, lb = inst
        k_, br = sub_offset(b_), sub_borrow(lb)
        oa, ob = slot_operands(a_, la, rnd), slot_operands(b_, lb, rnd)
        for (x, a), (y, b) in itertools.product(oa.items(), ob.items()):
            note = x + "," + y
            cases.append(Case("sums", "add", _inst(inst), a + b,
                              lambda out, w=val(a) + val(b), bd=a_ + b_, lm=la + lb: check_elem(out, w, bound=bd, limb=lm), note))
            cases.append(Case("sums", "sub", _inst(inst), a + b,
                              lambda out, w=val(a) - val(b), bd=a_ + k_, lm=la + br + 1: check_elem(out, w, bound=bd, limb=lm), note))
            cases.append(Case("sums", "sub_is_zero", _inst(inst), a + b, _flag((val(a) - val(b)) % P == 0), note))
        # operands k p apart, for every k the two types admit: a = b + k p (k >= 0) or b = a + |k| p; then one more and one less
        for k in range(-(b_ - 1), a_):
            if k >= 0:
                vb = rnd.randrange(min(b_, a_ - k) * P)
                va = vb + k * P
            else:
                va = rnd.randrange(min(a_, b_ + k) * P)
                vb = va - k * P
            assert 0 <= va < a_ * P and 0 <= vb < b_ * P
            for d in (0, 1, -1):
                if not 0 <= va + d < a_ * P:
                    continue
                cases.append(Case("sums", "sub_is_zero", _inst(inst), lazy(va + d, la, rnd) + lazy(vb, lb, rnd), _flag(d == 0),
                                  "%d p apart %+d" % (k, d)))
    for inst in UN_INSTS:
        a_, la = inst
        k_, br = sub_offset(a_), sub_borrow(la)
        oa = slot_operands(a_, la, rnd)
        ops = list(oa.items()) + [("rnd", lazy(rnd.randrange(a_ * P), la, rnd))]
        for note, a in ops:
            v = val(a)
            literal_zero = not any(a)
            cases.append(Case("sums", "dbl", _inst(inst), a, lambda out, v=v, a_=a_, la=la: check_elem(out, 2 * v, bound=2 * a_, limb=2 * la), note))
            # neg and cneg(., true) of the literal zero return exactly K p: the one input where the value bound holds with equality
            cases.append(Case("sums", "neg", _inst(inst), a,
                              lambda out, v=v, z=literal_zero, k_=k_, br=br: check_elem(out, -v, bound=k_, limb=br + 1, allow_equal=z), note))
            cases.append(Case("sums", "cneg", _inst(inst), a + [1],
                              lambda out, v=v, z=literal_zero, k_=k_, lm=max(br + 1, la): check_elem(out, -v, bound=k_, limb=lm, allow_equal=z),
                              note + ",true"))
            cases.append(Case("sums", "cneg", _inst(inst), a + [0],
                              lambda out, v=v, k_=k_, lm=max(br + 1, la): check_elem(out, v, bound=k_, limb=lm), note + ",false"))
            cases.append(Case("sums", "normed", _inst(inst), a, lambda out, v=v, a_=a_: check_elem(out, v, bound=a_, limb=1), note))
            cases.append(Case("sums", "is_zero", _inst(inst), a, _flag(v % P == 0), note))
            cases.append(Case("sums", "is_literal_zero", _inst(inst), a, _flag(literal_zero), note))
        for k in range(a_):
            for a in (normal(k * P), lazy(k * P, la, rnd)):
                cases.append(Case("sums", "is_zero", _inst(inst), a, _flag(True), "%d p" % k))
                cases.append(Case("sums", "is_literal_zero", _inst(inst), a, _flag(k == 0), "%d p" % k))
            for d in (1, -1):
                if 0 <= k * P + d < a_ * P:
                    cases.append(Case("sums", "is_zero", _inst(inst), lazy(k * P + d, la, rnd), _flag(False), "%d p %+d" % (k, d)))
    return cases


# ---- C. conversions --------------------------------------------------------------------------------------------------------------
CONV_INSTS = [(2, 1), (14, 3), (2048, 1), (45, 14)]


def _words_are(want):
    def check(out):
        assert out == want, ("words", ["%x" % w for w in out], ["%x" % w for w in want])
    return check


def conversions(rnd, mode):
    cases = []
    raws = [0, 1, P - 1, P, P + 1, (1 << 384) - 1] + [rnd.getrandbits(384) for _ in range(10)]
    for raw in raws:
        cases.append(Case("conversions", "from_raw", "-", words(raw, 12),
                          lambda out, raw=raw: check_elem(out, raw * RADIX, bound=2, limb=1), "%x" % raw))
        cases.append(Case("conversions", "raw_roundtrip", "-", words(raw, 12), _words_are(words(raw % P, 12)), "%x" % raw))
    for inst in CONV_INSTS:
        a_, la = inst
        oa = slot_operands(a_, la, rnd)
        ops = list(oa.items()) + [("rnd", lazy(rnd.randrange(a_ * P), la, rnd)) for _ in range(3)]
        ops += [("canonical %d" % c, normal(c * RADIX % P)) for c in (1, P - 1)]
        for note, a in ops:
            x = val(a) * RINV % P      # the element a stands for
            cases.append(Case("conversions", "to_raw", _inst(inst), a, _words_are(words(x, 12)), note))
            xi = pow(x, -1, P) if x else 0
            for op in ("inv", "inv_fermat"):
                cases.append(Case("conversions", op, _inst(inst), a, lambda out, xi=xi: check_elem(out, xi * RADIX, bound=2, limb=1), note))
            cases.append(Case("conversions", "pow_sqrt", _inst(inst), a,
                              lambda out, x=x: check_elem(out, pow(x, SQRT_E, P) * RADIX, bound=2, limb=1), note))
    return cases


# ---- D. group law ----------------------------------------------------------------------------------------------------------------
def aff_add(p, q):
    """the affine group law on y^2 = x^3 + 4; None is the point at infinity"""
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def aff_mul(k, p):
    acc = None
    for bit in bin(k)[2:]:
        acc = aff_add(acc, acc)
        if bit == "1":
            acc = aff_add(acc, p)
    return acc


def aff_neg(p):
    return p[0], (P - p[1]) % P


def xyzz_words(pt, z, jx, jy, fzz, fzzz):
    """X = x zz R + jx p, Y = y zzz R + jy p, ZZ = zz R (+ p), ZZZ = zzz R (+ p): normalised limbs, as an accumulator's members are"""
    zz, zzz = z * z % P, z * z * z % P
    vals = (pt[0] * zz * RADIX % P + jx * P, pt[1] * zzz * RADIX % P + jy * P, zz * RADIX % P + fzz * P, zzz * RADIX % P + fzzz * P)
    return [w for v in vals for w in normal(v)]


def affine_words(pt, fx, fy):
    return normal(pt[0] * RADIX % P + fx * P) + normal(pt[1] * RADIX % P + fy * P)


INFINITY_WORDS = [0] * 56


def check_point(want):
    def check(out):
        assert len(out) == 56
        x, y, zz, zzz = (out[14 * i:14 * i + 14] for i in range(4))
        if want is None:
            assert not any(zz), "a result at infinity has ZZ literally zero"
            return
        assert any(zz), "infinity returned for a finite sum"
        vx, vy, vzz, vzzz = val(x), val(y), val(zz), val(zzz)
        assert vzz % P and vzzz % P
        assert vx * pow(vzz, -1, P) % P == want[0], "X / ZZ"
        assert vy * pow(vzzz, -1, P) % P == want[1], "Y / ZZZ"
        assert pow(vzz * RINV, 3, P) == pow(vzzz * RINV, 2, P), "ZZ^3 = ZZZ^2"
        assert vx < 14 * P and vy < 6 * P and vzz < 2 * P and vzzz < 2 * P, ("value bounds", vx // P, vy // P, vzz // P, vzzz // P)
        assert all(l <= MASK for m in (x, y, zz, zzz) for l in m[:13]), "limbs 0..12 < 2^28"
    return check


def accumulator_shapes():
    """(jx, jy, ZZ + p?, ZZZ + p?): every multiple the members' types admit on X, the ends and one more on Y"""
    return [(jx, jy, fzz, fzzz) for jx in range(14) for jy in sorted({0, jx % 6, 5}) for fzz in (0, 1) for fzzz in (0, 1)]


def group(rnd, mode):
    cases = []
    g = (GX, GY)
    pairs = [(aff_mul(rnd.randrange(1, R), g), aff_mul(rnd.randrange(1, R), g)) for _ in range(3)]
    shapes = accumulator_shapes()
    flags = [(0, 0), (1, 0), (0, 1), (1, 1)]
    n = 0

    def add(op, inl, operand_words, want, note):
        cases.append(Case("group", op, str(inl), operand_words, check_point(want), note))

    for inl in (0, 1):
        for pi, (p, q) in enumerate(pairs):
            for op in ("xyzz_madd", "xyzz_madd_split") if pi == 0 else ("xyzz_madd",):
                # every shape on the first pair's xyzz_madd; elsewhere a quarter of them, the ZZ / ZZZ offsets rotating
                for shape in shapes if (pi == 0 and op == "xyzz_madd") else [s for i, s in enumerate(shapes) if (i + i // 4) % 4 == pi]:
                    acc = xyzz_words(p, rnd.randrange(1, P), *shape)
                    for b, what in ((q, "P+Q"), (p, "P+P"), (aff_neg(p), "P-P")):
                        n += 1
                        add(op, inl, acc + affine_words(b, *flags[n % 4]), aff_add(p, b), "%s %s" % (what, shape))
                for fx, fy in flags:   # the accumulator at infinity: ZZ literally zero, whatever the other members hold
                    add(op, inl, INFINITY_WORDS + affine_words(q, fx, fy), q, "O+Q")
                    junk = xyzz_words(p, rnd.randrange(1, P), 13, 5, 0, 1)
                    add(op, inl, junk[:28] + [0] * 14 + junk[42:] + affine_words(q, fx, fy), q, "O+Q, stale members")
        for i, shape in enumerate(shapes):
            p, q = pairs[i % 3]
            a = xyzz_words(p, rnd.randrange(1, P), *shape)
            other = shapes[(7 * i + 3) % len(shapes)]
            for b, what in ((q, "P+Q"), (p, "P+P"), (aff_neg(p), "P-P")):
                add("xyzz_add", inl, a + xyzz_words(b, rnd.randrange(1, P), *other), aff_add(p, b), "%s %s %s" % (what, shape, other))
            add("xyzz_dbl", inl, a, aff_add(p, p), str(shape))
            if i % 8 == 0:
                add("xyzz_add", inl, a + INFINITY_WORDS, p, "P+O")
                add("xyzz_add", inl, INFINITY_WORDS + a, p, "O+P")
        add("xyzz_add", inl, INFINITY_WORDS + INFINITY_WORDS, None, "O+O")
        add("xyzz_dbl", inl, INFINITY_WORDS, None, "2 O")
        for p, q in pairs:
            for pt in (p, q):
                for fx, fy in flags:
                    add("xyzz_dbl_affine", inl, affine_words(pt, fx, fy), aff_add(pt, pt), "%d %d" % (fx, fy))
    return cases


# ---- E. scalar side --------------------------------------------------------------------------------------------------------------
# (value bound in units of r, limb bound in units of 2^28) per operand. fr28.cuh: limb-bound product <= 24, value-bound product <= 2^25,
# a limb holds 15 units at most. A value < V r can saturate limbs of L units only if V r > L 2^252, i.e. L < 7.24 V.
FR28_MUL_BOUNDS = [(2, 1, 2, 1), (1 << 25, 1, 1, 1), (1, 1, 1 << 25, 1), (1 << 13, 4, 1 << 12, 6), (2, 12, 2, 2), (1 << 20, 8, 32, 3),
                   (8, 15, 4, 1), (2, 1, 1 << 24, 15), (4096, 6, 8192, 4)]
FR28_LAZY_BOUNDS = [(2, 1), (8, 15), (1 << 25, 1), (1 << 25, 15)]          # a factor of a constant (limb bound 1, value bound 1)
FR28_CONSTS = {"TO28": pow(2, 304, R), "NINV_RAW": pow(4096, -1, R), "TO256": pow(2, 256, R), "RR": pow(2, 560, R), "ONE": RADIX28 % R,
               "R3": pow(2, 840, R), "NINV_M": RADIX28 * pow(4096, -1, R) % R}
R28INV = pow(RADIX28, -1, R)


def check_fr28(want, value_bound=2, limb_bound=1, exact=False):
    def check(out):
        assert len(out) == 10
        v = val(out)
        if exact:
            assert v == want, "value differs"
        else:
            assert v % R == want % R, "value differs mod r"
            assert v < value_bound * R, ("value bound", v // R)
        assert all(l < limb_bound << W for l in out[:9]), ("limb bound", limb_bound)
    return check


def scalar(rnd, mode):
    cases = []

    def ops28(v, l):
        return slot_operands(v, l, rnd, R, 10)

    for bounds in FR28_MUL_BOUNDS:
        va, la, vb, lb = bounds
        assert la * lb <= 24 and va * vb <= 1 << 25 and la <= 15 and lb <= 15
        for (x, a), (y, b) in itertools.product(ops28(va, la).items(), ops28(vb, lb).items()):
            cases.append(Case("scalar", "fr28_mul", "-", a + b, check_fr28(val(a) * val(b) * R28INV), "%s %s*%s" % (bounds, x, y)))
    for va, la, vb, lb in [(2, 1, 2, 1), (4, 7, 4, 8), (1 << 24, 13, 3, 2)]:
        for (x, a), (y, b) in itertools.product(ops28(va, la).items(), ops28(vb, lb).items()):
            cases.append(Case("scalar", "fr28_add", "-", a + b, check_fr28(val(a) + val(b), limb_bound=la + lb, exact=True), x + "+" + y))
    for va, la in [(2, 1), (16, 13), (1 << 25, 13)]:      # a - b: b a product's result (normalised, < 4r); limb bound + 2
        for (x, a), (y, b) in itertools.product(ops28(va, la).items(), ops28(4, 1).items()):
            cases.append(Case("scalar", "fr28_sub", "-", a + b, check_fr28(val(a) + 4 * R - val(b), limb_bound=la + 2, exact=True), x + "-" + y))
    for va, la in [(2, 1), (8, 15), (1 << 25, 15)]:
        for x, a in ops28(va, la).items():
            cases.append(Case("scalar", "fr28_norm", "-", a, check_fr28(val(a), exact=True), x))
    for v in [0, 1, R - 1, R, R + 1, 2 * R - 1] + [rnd.randrange(2 * R) for _ in range(6)]:
        cases.append(Case("scalar", "fr28_canonical", "-", normal(v, 10), _words_are(normal(v % R, 10)), "%x" % v))
    for va, la in FR28_LAZY_BOUNDS:
        for x, a in list(ops28(va, la).items()) + [("rnd", lazy(rnd.randrange(va * R), la, rnd, 10))]:
            y = val(a) * R28INV % R      # the scalar a stands for
            cases.append(Case("scalar", "fr28_to_raw_scaled", "-", a, _words_are(words(y * pow(4096, -1, R) % R, 8)), x))
            cases.append(Case("scalar", "fr28_to_mont256", "-", a, _words_are(words(y * (1 << 256) % R, 8)), x))
            for name, c in FR28_CONSTS.items():
                cases.append(Case("scalar", "fr28_mul_const", name, a, check_fr28(val(a) * c * R28INV), x))
    for x in [0, 1, R - 1] + [rnd.randrange(R) for _ in range(5)]:     # x: the canonical words of a Montgomery form (x 2^256)
        cases.append(Case("scalar", "fr28_from_mont256", "-", words(x, 8), check_fr28(x << 24), "%x" % x))
    for name, mod, n in (("fp", P, 12), ("fr", R, 8)):
        mr = 1 << (32 * n)
        mrinv = pow(mr, -1, mod)
        elems = [0, 1, mod - 1] + [rnd.randrange(mod) for _ in range(3)]

        def is_(v, n=n):
            return _words_are(words(v, n))

        for a, b in itertools.product(elems, elems):
            cases.append(Case("scalar", name + "_mul", "-", words(a, n) + words(b, n), is_(a * b * mrinv % mod)))
            cases.append(Case("scalar", name + "_add", "-", words(a, n) + words(b, n), is_((a + b) % mod)))
            cases.append(Case("scalar", name + "_sub", "-", words(a, n) + words(b, n), is_((a - b) % mod)))
        for a in elems + [mr % mod, rnd.randrange(mod), rnd.randrange(mod)]:
            cases.append(Case("scalar", name + "_neg", "-", words(a, n), is_(-a % mod)))
            cases.append(Case("scalar", name + "_sqr", "-", words(a, n), is_(a * a * mrinv % mod)))
            ai = mr * mr * pow(a, -1, mod) % mod if a else 0      # (v R)^-1 in Montgomery form
            for op in ("_inv", "_inv_fermat" if name == "fp" else "_inv_divsteps"):
                cases.append(Case("scalar", name + op, "-", words(a, n), is_(ai)))
    ks = [0, Z2 - 1, Z2, R - 1, (1 << 256) - 1]
    for m in (1, 1 << 127, Z2 - 1):
        ks += [m * Z2, m * Z2 + 1, m * Z2 - 1]
    ks += [rnd.getrandbits(256) for _ in range(64)]
    for k in ks:
        hi, lo = divmod(k, Z2)
        # the quotient is returned in four words: beyond z^2 2^128 (no scalar: r < 2^255) its low 128 bits are what they can hold
        want = words(lo, 4) + words(hi & ((1 << 128) - 1), 4)
        for op in ("split_by_z2", "split_by_z2_barrett"):
            cases.append(Case("scalar", op, "-", words(k, 8), _words_are(want), "%x" % k))
    return cases


CHECKER_UNITS = ("A", "B", "C", "D", "Di", "E", None)      # -DPC_FAM of tests/prims_check.hip's translation units; None: main()


def build_checker(root, out_dir, host_only):
    """compiles tests/prims_check.hip with the flags of csrc/Makefile, its seven translation units side by side, and links them.
    Returns (path of the program, seconds the build took), or (None, 0) where there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None, 0.0
    flags = ["-DLWK_LIMB_BITS=28", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(root, "lambdaworks_kzg_amd", "csrc")]
    if host_only:
        flags += ["--cuda-host-only", "-DPRIMS_HOST_ONLY"]
    src = os.path.join(root, "tests", "prims_check.hip")
    t0 = time.time()
    jobs, objs = [], []
    for unit in CHECKER_UNITS:
        obj = os.path.join(out_dir, "prims_check_%s.o" % (unit or "main"))
        objs.append(obj)
        jobs.append(subprocess.Popen([hipcc] + flags + (["-DPC_FAM=" + unit] if unit else []) + ["-c", src, "-o", obj]))
    status = [j.wait() for j in jobs]
    assert not any(status), "prims_check.hip does not compile"
    exe = os.path.join(out_dir, "prims_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950"] + (["--cuda-host-only"] if host_only else []) + objs + ["-o", exe])
    return exe, time.time() - t0


def run_checker(exe, mode, work_dir, timeout):
    """one run of the checker over every case: a subprocess under a time limit, a non-zero exit raises, nothing is retried.
    Returns (cases, result lines, seconds)."""
    cases = build_cases(mode)
    cases_path, results_path = os.path.join(work_dir, "cases.txt"), os.path.join(work_dir, "results.txt")
    write_cases(cases_path, cases)
    t0 = time.time()
    subprocess.run([exe, mode, cases_path, results_path], check=True, timeout=timeout)
    seconds = time.time() - t0
    return cases, read_results(results_path), seconds


def build_cases(mode, seed=0x5eed29):
    """every case of every family, in file order. mode: "host" or "device" (the declared bound of the inlined mul_sub differs)"""
    assert mode in ("host", "device")
    out = []
    for i, family in enumerate((products, sums, conversions, group, scalar)):
        out += family(random.Random(seed + i), mode)
    return out


def write_cases(path, cases):
    with open(path, "w") as f:
        for c in cases:
            f.write(c.line + "\n")


def read_results(path):
    with open(path) as f:
        return [[int(w, 16) for w in line.split()] for line in f.read().split("\n")[:-1]]


def check_family(family, cases, results):
    """holds every result line of one family to its expectation; returns the number of cases checked"""
    assert len(results) == len(cases), (len(results), len(cases))
    bad, n = [], 0
    for c, out in zip(cases, results):
        if c.family != family:
            continue
        n += 1
        try:
            c.check(out)
        except AssertionError as e:
            bad.append("%r: %s" % (c, e))
    assert not bad, "%d of %d cases of family %s fail:\n%s" % (len(bad), n, family, "\n".join(bad[:12]))
    assert n > 0
    return n
