"""Blobs that make the commitment step's hand-scheduled kernels meet P = +-Q (and so raise their blob's redo flag), in one place: the
constructions, whole batches with such blobs at the indices where the launch sets change, and a plain integer model of the 256 lanes
of a workgroup that says, from the setup's secret alone, WHERE each construction collides (tests/test_flag_cases_cpu.py).

The setup's points are P_i = [k_i]G with k_i known: tau^i for tests/golden/trusted_setup.txt (tau = 1337), and for its Lagrange form,
in the bit-reversed order a c-kzg-mode MSM runs over, l_i(tau) = (tau^4096 - 1) / 4096 * w_i / (tau - w_i) with w_i = w^bitrev12(i).
With one workgroup per blob lane t owns the scalars t, t + 256, ... and adds one table row d_j 2^(c j) P_i per non-zero signed digit
d_j of each (direct.hip: direct_accumulate_blob); one fold wave then adds the 256 lane sums (tools/gen_fold_asm.py).
Test infrastructure, like proof_cases.py and fuzz_cases.py: nothing here touches the GPU."""
import collections
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import blobs as B  # noqa: E402

R = B.R
N = B.N
TAU = 1337   # the secret of tests/golden/trusted_setup.txt
LANES = 256
WIDTHS = (10, 11, 12, 13, 14, 15, 16)   # every direct-table width
# (a, b, others random): lanes a and b of a blob's one workgroup end with equal (odd blobs: opposite) sums and every other scalar of
# theirs is zero, so the pair meets in the FOLD, not in the accumulation: 3 and 67 are two of the four lane sums one fold thread adds in
# sequence, 5 and 37 meet at the first level of the tree, 5 and 6 at its last, 200 and 9 in between
FOLD_PAIRS = [(3, 67, True), (5, 37, True), (5, 6, False), (200, 9, False)]


def fold_collision_scalars(blob):
    """scalars of blob `blob` of the fold-collision batch (one workgroup per blob: lane t owns the scalars t, t + 256, ...)"""
    rnd = random.Random(88000 + blob)
    a, b, others = FOLD_PAIRS[(blob // 2) % len(FOLD_PAIRS)]
    ss = [0] * 4096
    if others:   # the lanes of other fold threads carry random sums; they join behind the level where a and b meet
        for i in range(4096):
            if (i % 256) % 64 not in (a % 64, b % 64):
                ss[i] = rnd.randrange(R)
    ss[a] = rnd.randrange(1, R)
    ss[b] = ss[a] * pow(TAU, a - b, R) % R       # s_b tau^b = s_a tau^a
    if blob % 2:
        ss[b] = (R - ss[b]) % R
    return ss


def one_colliding_lane_blob(rnd, c, negate):
    """Random full-range scalars, except that ONE lane of the direct kernel meets a table row equal to (negate: opposite to) its
    accumulator, once, late: with P_k = [tau^k]G, s_i = +-e tau^2048 (i < 256: the lane's first scalar in every launch geometry),
    s_(i + 256 m) = 0 for m = 1 .. 7 (skipped), s_(i + 2048) = e -- after the 255 bits of s_i the lane holds +-[e]P_(i + 2048) and the
    next row it gathers is [e]P_(i + 2048)."""
    ss = [rnd.randrange(R) for _ in range(4096)]
    i = rnd.randrange(256)
    e = rnd.randrange(1, 1 << (c - 1))
    for m in range(1, 8):
        ss[i + 256 * m] = 0
    ss[i + 2048] = e
    ss[i] = e * pow(TAU, 2048, R) % R
    if negate:
        ss[i] = (R - ss[i]) % R
    return ss


# ---- the points' discrete logarithms -------------------------------------------------------------------------------------------

_point_scalars = {}


def point_scalars(lagrange=False):
    """k_i with P_i = [k_i]G, in the order the MSM pairs them with a blob's elements"""
    if lagrange not in _point_scalars:
        if lagrange:
            import make_lagrange_setup as L
            nat = L.lagrange_scalars(TAU)
            _point_scalars[lagrange] = [nat[int(format(i, "012b")[::-1], 2)] for i in range(N)]
        else:
            ks, t = [], 1
            for _ in range(N):
                ks.append(t)
                t = t * TAU % R
            _point_scalars[lagrange] = ks
    return _point_scalars[lagrange]


def closed_form_scalar(scalars, lagrange=False):
    return sum(s * k for s, k in zip(scalars, point_scalars(lagrange))) % R


def closed_form(oracle, scalars, lagrange=False):
    """[sum s_i k_i]G compressed: [sum s_i tau^i]G, or on the Lagrange form [sum s_i l_i(tau)]G"""
    return oracle.g1_generator_mul(closed_form_scalar(scalars, lagrange))


# ---- special blobs ---------------------------------------------------------------------------------------------------------------

# the kinds of special blob: a collision in the accumulation, each fold pair, both at once, and two blobs with (next to) nothing to add
KINDS = (["acc_eq", "acc_opp"] + ["fold%d_%s" % (p, s) for p in range(len(FOLD_PAIRS)) for s in ("eq", "opp")] +
         ["acc_and_fold", "zero", "one_scalar"])
ACC_KINDS = ("acc_eq", "acc_opp", "acc_and_fold")
Special = collections.namedtuple("Special", "index kind scalars")


def _ratio(k, a, b):
    """k_a / k_b mod r"""
    return k[a] * pow(k[b], R - 2, R) % R


def _acc_collision(ss, rnd, k, negate, lanes):
    """one_colliding_lane_blob's construction over any point set and for every table width (e < 2^9: one digit of the narrowest)"""
    i = rnd.choice(lanes)
    e = rnd.randrange(1, 1 << 9)
    for m in range(1, 8):
        ss[i + 256 * m] = 0
    ss[i + 2048] = e
    ss[i] = e * _ratio(k, i + 2048, i) % R        # s_i k_i = e k_(i + 2048)
    if negate:
        ss[i] = (R - ss[i]) % R
    return i


def special_scalars(kind, seed, lagrange=False):
    """the 4096 scalars (integers below r) of a special blob of `kind`; `seed` picks its random choices"""
    rnd = random.Random("%s/%d/%d" % (kind, seed, int(lagrange)))
    k = point_scalars(lagrange)
    if kind == "zero":
        return [0] * N
    if kind == "one_scalar":
        ss = [0] * N
        ss[rnd.randrange(N)] = rnd.randrange(1, R)
        return ss
    if kind in ("acc_eq", "acc_opp"):
        ss = [rnd.randrange(R) for _ in range(N)]
        _acc_collision(ss, rnd, k, kind == "acc_opp", range(LANES))
        return ss
    pair = 0 if kind == "acc_and_fold" else int(kind[4])
    a, b, others = FOLD_PAIRS[pair]
    others = others or kind == "acc_and_fold"
    ss = [0] * N
    if others:
        for i in range(N):
            if (i % 256) % 64 not in (a % 64, b % 64):
                ss[i] = rnd.randrange(R)
    ss[a] = rnd.randrange(1, R)
    ss[b] = ss[a] * _ratio(k, a, b) % R           # s_b k_b = s_a k_a
    if kind.endswith("opp"):
        ss[b] = (R - ss[b]) % R
    if kind == "acc_and_fold":   # (the accumulation's flag wins: the second pass recomputes the blob and the tail skips its fold)
        _acc_collision(ss, rnd, k, True, [t for t in range(LANES) if t % 64 not in (a % 64, b % 64)])
    return ss


REQUIRED = (0, 1, 255, 256, 511, 512, 767)     # and n - 2, n - 1, and the ends of every chunk of 1024 a longer call is cut into
ROW_RUN = (77, 333, 589, 845)                  # congruent mod 256: one row of the second pass (256 rows) recomputes all four at n = 1024
N_SPECIAL = 40


def special_layout(n, seed):
    """[(index, kind)] of the special blobs of full_chunk_batch(n, seed), ascending"""
    assert n >= 1023, n
    rnd = random.Random(7100 + seed)
    fixed = set(REQUIRED) | {n - 2, n - 1} | {i for i in (1023, 1024, 2047, 2048) if i < n}
    kinds = {i: ACC_KINDS[j % len(ACC_KINDS)] for j, i in enumerate(ROW_RUN)}
    taken = fixed | set(ROW_RUN)
    # further specials at seeded indices, at least three honest blobs away from every other special
    while len(taken) < N_SPECIAL:
        i = rnd.randrange(n)
        if all(abs(i - j) > 3 for j in taken):
            taken.add(i)
    order = list(KINDS)
    rnd.shuffle(order)
    rest = sorted(taken - set(ROW_RUN))
    for j, i in enumerate(rest):
        kinds[i] = order[j % len(order)]
    return sorted(kinds.items())


def _encode(scalars, big_endian):
    order = "big" if big_endian else "little"
    return b"".join(s.to_bytes(32, order) for s in scalars)


_batches = {}


def full_chunk_batch(n, seed, lagrange=False):
    """(bytes of n blobs, [Special]): honest synthetic blobs (B.synthetic_blob(1000 seed + i)) with about forty special ones written over
    them. lagrange: the twins for c-kzg mode on the Lagrange form -- little-endian elements below r, the same collisions among the
    points [l_i(tau)]G. The result is cached and must not be modified."""
    key = (n, seed, lagrange)
    if key not in _batches:
        data = bytearray(b"".join(B.synthetic_blob(1000 * seed + i, big_endian=not lagrange) for i in range(n)))
        specials = []
        for index, kind in special_layout(n, seed):
            ss = special_scalars(kind, 1000 * seed + index, lagrange)
            data[index * B.BYTES_PER_BLOB:(index + 1) * B.BYTES_PER_BLOB] = _encode(ss, not lagrange)
            specials.append(Special(index, kind, ss))
        _batches[key] = (bytes(data), specials)
    return _batches[key]


def honest_sample(n, specials):
    """honest blobs to hold against the closed form: every 61st, the last one, and both neighbours of every special blob (a flag
    must not leak to a neighbour)"""
    special = {s.index for s in specials}
    near = {i for s in specials for i in (s.index - 1, s.index + 1) if 0 <= i < n}
    return sorted((set(range(0, n, 61)) | {n - 1} | near) - special)


def blob_scalars_at(data, index, lagrange=False):
    return B.blob_scalars(data[index * B.BYTES_PER_BLOB:(index + 1) * B.BYTES_PER_BLOB], big_endian=not lagrange)


def wrong_blobs(oracle, data, specials, got, lagrange=False):
    """indices among the special blobs and honest_sample whose 48 bytes in `got` are not the closed form"""
    n = len(data) // B.BYTES_PER_BLOB
    assert len(got) == 48 * n
    bad = [(s.index, s.kind) for s in specials if got[48 * s.index:48 * s.index + 48] != closed_form(oracle, s.scalars, lagrange)]
    for i in honest_sample(n, specials):
        if got[48 * i:48 * i + 48] != closed_form(oracle, blob_scalars_at(data, i, lagrange), lagrange):
            bad.append((i, "honest"))
    return bad


# ---- the lanes, as integers ------------------------------------------------------------------------------------------------------

def signed_digits(s, c):
    """the digits of direct_accumulate_blob: c-bit windows, a window above 2^(c-1) becomes negative and carries; the top one is unsigned"""
    nw = (255 + c - 1) // c
    h = 1 << (c - 1)
    out, carry = [], 0
    for j in range(nw):
        top = j == nw - 1
        raw = ((s >> (c * j)) & ((1 << (255 - c * (nw - 1) if top else c)) - 1)) + carry
        neg = (not top) and raw > h
        out.append(raw - (1 << c) if neg else raw)
        carry = 1 if neg else 0
    assert sum(d << (c * j) for j, d in enumerate(out)) == s
    return out


def lane_sums(scalars, lagrange=False, lanes_per_blob=LANES):
    """discrete logarithms of the lane sums: lane t owns the scalars t, t + lanes_per_blob, ..."""
    k = point_scalars(lagrange)
    return [sum(scalars[i] * k[i] for i in range(t, N, lanes_per_blob)) % R for t in range(lanes_per_blob)]


def lane_chain_collisions(scalars, c, lanes, lagrange=False, lanes_per_blob=LANES):
    """[(lane, point, window, sign)]: the additions of the accumulation in which a lane's non-zero partial sum equals (sign +1) or is
    opposite to (-1) the row it adds next, on the table of width c"""
    k = point_scalars(lagrange)
    out = []
    for t in lanes:
        acc = 0
        for i in range(t, N, lanes_per_blob):
            if not scalars[i]:
                continue
            base = k[i]
            for j, d in enumerate(signed_digits(scalars[i], c)):
                if d:
                    row = d * base % R
                    if acc and acc == row:
                        out.append((t, i, j, 1))
                    elif acc and acc + row == R:
                        out.append((t, i, j, -1))
                    acc = (acc + row) % R
                base = (base << c) % R
    return out


def coinciding_lanes(sums):
    """[(a, b, sign)], a < b: pairs of non-zero lane sums that are equal (+1) or opposite (-1)"""
    seen, out = {}, []
    for t, v in enumerate(sums):
        if not v:
            continue
        for key, sign in ((v, 1), (R - v, -1)):
            if key in seen:
                out.append((seen[key], t, sign))
        seen.setdefault(v, t)
    return out
