"""EIP-7594 recover_cells_and_kzg_proofs restated in Python over tests/cells_spec.py, two ways. Test helper only.

recover_polynomialcoeff: the consensus-specs route -- the vanishing polynomial of the missing cells spread by 64, E Z on the
extended domain, an 8192-point inverse transform, the division on the coset of 7, and back. It returns all 8192 coefficients: the
upper 4096 are zero exactly when a polynomial of degree < 4096 through the given cells exists.

recover_factored: what csrc/recover.hip computes. With p(X) = sum_{t<64} X^t P_t(X^64) the interpolant of cell k on its coset is
I_k = p mod (X^64 - c_k) and I_k[t] = P_t(c_k): 64 erasure decodings of a polynomial of degree < 64 over the 128th roots of unity,
all with the same erasure pattern. It returns (coefficients, upper): Q_t's coefficients 0 .. 63 spread to 64 m + t, and its
coefficients 64 .. 127 (all zero exactly when the cells are consistent)."""
import cells_spec as S

R = S.R
GEN = 7   # the coset both routes divide on
W128 = pow(7, (R - 1) // 128, R)
W64 = pow(7, (R - 1) // 64, R)


def inv(x):
    return pow(x, R - 2, R)


def intt(a, w):
    n_inv = inv(len(a))
    return [x * n_inv % R for x in S.ntt(list(a), inv(w))]


def recover_polynomialcoeff(cell_indices, cells_values):
    """cells_values[i]: the 64 integers of cell cell_indices[i]. The 8192 coefficients of the spec's reconstruction."""
    given = set(cell_indices)
    missing = [k for k in range(S.N_CELLS) if k not in given]
    # Z(X) = prod over the missing cells of (X^64 - c_k): the 128-point vanishing polynomial in Y = X^64, spread by 64
    short = S.vanishing_polynomialcoeff([S.c_of_cell(k) for k in missing])
    z = [0] * S.N_EXT
    for i, c in enumerate(short):
        z[64 * i] = c
    z_eval = S.brp(S.ntt(z, S.W8192))               # Z on D, in the cells' order
    e_eval = [0] * S.N_EXT
    for k, vals in zip(cell_indices, cells_values):
        e_eval[64 * k:64 * k + 64] = vals
    ez_eval = [a * b % R for a, b in zip(e_eval, z_eval)]
    ez = intt(S.brp(ez_eval), S.W8192)              # (E Z)(X), degree < 8192
    shift = [1] * S.N_EXT
    for i in range(1, S.N_EXT):
        shift[i] = shift[i - 1] * GEN % R
    ez_coset = S.ntt([c * s % R for c, s in zip(ez, shift)], S.W8192)
    z_coset = S.ntt([c * s % R for c, s in zip(z, shift)], S.W8192)
    q_coset = [a * inv(b) % R for a, b in zip(ez_coset, z_coset)]
    q = intt(q_coset, S.W8192)
    return [c * inv(s) % R for c, s in zip(q, shift)]


def cell_interpolant(k, vals):
    """the 64 coefficients of the polynomial of degree < 64 through cell k's values on its coset h_k <w64>, h_k = w8192^bitrev7(k)"""
    h_inv = inv(pow(S.W8192, S.rev(k, 7), R))
    coeffs = intt(S.brp(list(vals)), W64)           # of I_k(h_k X)
    out, s = [], 1
    for c in coeffs:
        out.append(c * s % R)
        s = s * h_inv % R
    return out


def recover_tables(cell_indices):
    """what k_recover_setup leaves for one index set: Zs(w128^q) and 1 / Zs(7 w128^q) for q < 128, Zs(Y) = prod over the missing cells of (Y - c_k)"""
    given = set(cell_indices)
    miss_roots = [S.c_of_cell(k) for k in range(S.N_CELLS) if k not in given]

    def zs(y):
        acc = 1
        for c in miss_roots:
            acc = acc * (y - c) % R
        return acc

    roots = [pow(W128, q, R) for q in range(128)]
    return [zs(x) for x in roots], [inv(zs(GEN * x % R)) for x in roots]


def recover_factored(cell_indices, cells_values):
    zs_root, zs_coset_inv = recover_tables(cell_indices)
    interp = {k: cell_interpolant(k, v) for k, v in zip(cell_indices, cells_values)}
    coeffs, upper = [0] * S.N_BLOB, []
    g_pow = [pow(GEN, j, R) for j in range(128)]
    for t in range(64):
        e = [0] * 128                                # position q = bitrev7(k): the value at w128^q, times Zs there
        for k in cell_indices:
            q = S.rev(k, 7)
            e[q] = interp[k][t] * zs_root[q] % R
        n_t = intt(e, W128)                          # P_t Zs, degree < 128
        v = S.ntt([c * g % R for c, g in zip(n_t, g_pow)], W128)
        q_t = intt([a * b % R for a, b in zip(v, zs_coset_inv)], W128)
        q_t = [c * inv(g) % R for c, g in zip(q_t, g_pow)]
        for m in range(64):
            coeffs[64 * m + t] = q_t[m]
        upper.append(q_t[64:])
    return coeffs, upper
