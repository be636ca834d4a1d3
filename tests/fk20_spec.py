"""The FK20 route to the 128 cell proofs of a blob restated in Python over tests/cells_spec.py. Everything is
linear in the setup points, so the "group" here is any module over the integers mod r given by its points: the integers mod r under
addition (a point is an int, [k]P is k * P % R) stand in for G1. Test helper only.

    h_u     = sum_{t < 4096 - 64 (u + 1)} p[t + 64 (u + 1)] G[t],  u < 64  (h_63 = O)
    proof_k = sum_{u < 64} c_k^u h_u = F[rev7(k)],  F the forward 128-point transform (root w) of (h_0 .. h_63, O x 64)
  setup side:  Y_i[j] = G[64 (62 - j) + i] for j <= 62, O for 63 <= j < 128;  Y^_i = the forward transform of Y_i
  blob side:   A_i[0] = p[4032 + i], A_i[m] = 0 for 1 <= m <= 65, A_i[m] = p[64 (m - 65) + i] for 66 <= m <= 127;  A^_i its transform
               E[m] = sum_i A^_i[m] Y^_i[m];  (h_0 .. h_127) = the inverse transform of E, entries 64 .. 127 replaced by O"""
import cells_spec as S

R = S.R
N, T = 128, 64
W = pow(7, (R - 1) // N, R)     # the library's w128


def transform(values, root):
    """[sum_j values[j] root^(i j) for i < len(values)] over ints mod r (scalars, or points of the toy group)"""
    return S.ntt(list(values), root)


def h_direct(p, G):
    return [sum(p[t + T * (u + 1)] * G[t] for t in range(S.N_BLOB - T * (u + 1))) % R for u in range(T)]


def bases(G):
    """Y^_i[m] at [i][m]"""
    out = []
    for i in range(T):
        y = [G[T * (62 - j) + i] if j <= 62 else 0 for j in range(N)]
        out.append(transform(y, W))
    return out


def coefficient_rows(p):
    """A_i at [i]"""
    return [[p[4032 + i]] + [0] * 65 + [p[T * (m - 65) + i] for m in range(66, N)] for i in range(T)]


def coefficient_transforms(p):
    return [transform(a, W) for a in coefficient_rows(p)]


def e_points(p, yhat):
    ahat = coefficient_transforms(p)
    return [sum(ahat[i][m] * yhat[i][m] for i in range(T)) % R for m in range(N)]


def h_from_e(e):
    inv_n = pow(N, R - 2, R)
    full = [x * inv_n % R for x in transform(e, pow(W, R - 2, R))]
    return full[:T], full[T:]


def proofs_from_h(h):
    f = transform(list(h) + [0] * (N - T), W)
    return [f[S.rev(k, 7)] for k in range(N)]


def proofs(p, G):
    h, _ = h_from_e(e_points(p, bases(G)))
    return proofs_from_h(h)


def proofs_by_quotients(p, G):
    """the definition: proof_k = the commitment of q_k = p div (X^64 - c_k)"""
    return [sum(q * g for q, g in zip(S.quotient(p, k), G)) % R for k in range(N)]


def edge_polynomial(tau):
    """X^64 - tau^64 X^2048 + X^2112: on a powers-of-tau setup h_0 = h_32 = G and every other h_u is at infinity, so the forward
    transform doubles in one butterfly and cancels in another; proof_k = [1 + (w^32)^rev7(k)]G"""
    p = [0] * S.N_BLOB
    p[64] = 1
    p[2048] = (-pow(tau, 64, R)) % R
    p[2112] = 1
    return p
