"""EIP-7594 verify_cell_kzg_proof_batch restated in Python over ints and hashlib, in the settings' mode as DESIGN.md section 4i defines
it: de-duplication, the two-level transcript, the interpolant of a cell on its coset by two routes, the four sums of the check with
the oracle's G1 arithmetic, and the check itself done in G1 with tau known (no pairing). Test helper only.

An item is (commitment 48 bytes, cell index, cell 2048 bytes, proof 48 bytes)."""
import hashlib

import cells_spec as S
from cells_spec import R

DOMAIN = b"RCKZGCBATCH__V1_"


def dedupe(commitments):
    """distinct commitments by byte equality in order of first occurrence, and the row index of every item"""
    distinct, rows, seen = [], [], {}
    for c in commitments:
        c = bytes(c)
        if c not in seen:
            seen[c] = len(distinct)
            distinct.append(c)
        rows.append(seen[c])
    return distinct, rows


def item_digest(row, k, cell, proof):
    return hashlib.sha256(row.to_bytes(8, "little") + k.to_bytes(8, "little") + bytes(cell) + bytes(proof)).digest()


def challenge(items, mode):
    """r of the batch: the digest of the header, the distinct commitments and the per-item digests, read in the mode's byte order, mod r"""
    distinct, rows = dedupe([it[0] for it in items])
    msg = DOMAIN + (4096).to_bytes(8, "little") + (64).to_bytes(8, "little") + len(distinct).to_bytes(8, "little") + \
        len(items).to_bytes(8, "little") + b"".join(distinct)
    for row, (_, k, cell, proof) in zip(rows, items):
        msg += item_digest(row, k, cell, proof)
    return int.from_bytes(hashlib.sha256(msg).digest(), "little" if mode == S.MODE_CKZG else "big") % R


def cell_elements(cell, mode):
    return [S.element(cell[32 * t:32 * t + 32], mode) for t in range(S.N_CELL)]


def interpolant(cell_values, k):
    """coefficients of the degree-< 64 polynomial that takes cell_values[t] at coset_for_cell(k)[t]: Lagrange's formula, literally"""
    xs = S.coset_for_cell(k)
    out = [0] * S.N_CELL
    for j, xj in enumerate(xs):
        num = S.vanishing_polynomialcoeff(xs[:j] + xs[j + 1:])
        den = 1
        for i, xi in enumerate(xs):
            if i != j:
                den = den * (xj - xi) % R
        f = cell_values[j] * pow(den, R - 2, R) % R
        for t in range(S.N_CELL):
            out[t] = (out[t] + f * num[t]) % R
    return out


def interpolant_by_transform(cell_values, k):
    """the same by the route the kernel takes: the values are the evaluations of J(Y) = I(h Y) at w64^bitrev6(t), h = D[64 k]; an
    inverse 64-point transform gives J's coefficients and coefficient t of I is that of J over h^t"""
    h = pow(S.W8192, S.rev(S.N_CELL * k, 13), R)
    w64 = pow(7, (R - 1) // S.N_CELL, R)
    nat = S.brp(list(cell_values))
    j = [c * pow(S.N_CELL, R - 2, R) % R for c in S.ntt(nat, pow(w64, R - 2, R))]
    hi = pow(h, R - 2, R)
    return [c * pow(hi, t, R) % R for t, c in enumerate(j)]


def _point(oracle, b48):
    p = oracle.g1_decompress(bytes(b48))
    assert p is not None, "not a point of G1"
    return p


def _add(oracle, a, b):
    return oracle.g1_add_affine(a[0], a[1], b[0], b[1])


def _mul(oracle, p, k):
    if p[1] or k % R == 0:
        return (bytes(96), True)
    return oracle.g1_mul_affine(p[0], k % R)


def _neg(p):
    if p[1]:
        return p
    y = (S_P - int.from_bytes(p[0][48:], "big")) % S_P
    return (p[0][:48] + y.to_bytes(48, "big"), False)


S_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
INF = (bytes(96), True)


def sums(oracle, items, mode, tau):
    """r and the four sums P, RLC, RLI, RLP as affine points (xy 96 bytes, is_infinity)"""
    r = challenge(items, mode)
    distinct, rows = dedupe([it[0] for it in items])
    weights = [0] * len(distinct)
    p_sum, rlp, i_tau = INF, INF, 0
    a = 1
    for row, (_, k, cell, proof) in zip(rows, items):
        pi = _point(oracle, proof)
        p_sum = _add(oracle, p_sum, _mul(oracle, pi, a))
        rlp = _add(oracle, rlp, _mul(oracle, pi, a * S.c_of_cell(k)))
        weights[row] = (weights[row] + a) % R
        i_tau = (i_tau + a * S.evaluate(interpolant_by_transform(cell_elements(cell, mode), k), tau)) % R
        a = a * r % R
    rlc = INF
    for c, w in zip(distinct, weights):
        rlc = _add(oracle, rlc, _mul(oracle, _point(oracle, c), w))
    rli = _point(oracle, oracle.g1_generator_mul(i_tau))
    return r, p_sum, rlc, rli, rlp


def partials(oracle, items, mode, tau):
    """r and the four sums as compressed points"""
    r, *pts = sums(oracle, items, mode, tau)
    return (r,) + tuple(oracle.g1_compress(xy, inf) for xy, inf in pts)


def partials_bytes(oracle, items, mode, tau):
    """the layout of lwkzg_cell_verify_partials: r 32 (the mode's byte order) | P | RLC | RLI | RLP, each flag 1 | x 48 | y 48"""
    r, *pts = sums(oracle, items, mode, tau)
    out = S.to_bytes(r, mode)
    for xy, inf in pts:
        out += (b"\x01" + bytes(96)) if inf else (b"\x00" + xy)
    return out


def verdict_known_tau(oracle, items, mode, tau):
    """the batch check in G1 with tau known: RLC - RLI + RLP == [tau^64] P"""
    _, p_sum, rlc, rli, rlp = sums(oracle, items, mode, tau)
    lhs = _add(oracle, _add(oracle, rlc, _neg(rli)), rlp)
    rhs = _mul(oracle, p_sum, pow(tau, 64, R))
    return (lhs[1] and rhs[1]) or (lhs[1] == rhs[1] and lhs[0] == rhs[0])


def item_holds_known_tau(oracle, item, mode, tau):
    """one item: C - [I(tau)]G == [tau^64 - c_k] pi"""
    c, k, cell, proof = item
    i_tau = S.evaluate(interpolant_by_transform(cell_elements(cell, mode), k), tau)
    lhs = _add(oracle, _point(oracle, c), _neg(_point(oracle, oracle.g1_generator_mul(i_tau))))
    rhs = _mul(oracle, _point(oracle, proof), (pow(tau, 64, R) - S.c_of_cell(k)) % R)
    return (lhs[1] and rhs[1]) or (lhs[1] == rhs[1] and lhs[0] == rhs[0])
