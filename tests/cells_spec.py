"""EIP-7594 cells and cell proofs restated in Python (the consensus-specs polynomial-commitments-sampling text, over Python ints):
the extended domain, cells by an 8192-point transform, the spec's coset_for_cell / vanishing_polynomialcoeff / divide_polynomialcoeff,
and a fast quotient (the binomial recurrence) that tests/test_cells_cpu.py holds against the spec's long division. Test helper only."""
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N_BLOB, N_EXT, N_CELL, N_CELLS = 4096, 8192, 64, 128
W8192 = pow(7, (R - 1) // N_EXT, R)
W4096 = pow(7, (R - 1) // N_BLOB, R)
MODE_REFERENCE, MODE_CKZG = 0, 1


def rev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


def brp(values):
    bits = len(values).bit_length() - 1
    return [values[rev(i, bits)] for i in range(len(values))]


def roots(n):
    w = pow(7, (R - 1) // n, R)
    out, x = [], 1
    for _ in range(n):
        out.append(x)
        x = x * w % R
    return out


def ntt(a, w):
    """[a(w^i) for i < len(a)], natural order, w a primitive len(a)-th root of unity (iterative radix 2)"""
    n = len(a)
    bits = n.bit_length() - 1
    v = [a[rev(i, bits)] for i in range(n)]
    half = 1
    while half < n:
        wl = pow(w, n // (2 * half), R)
        tw = [1] * half
        for k in range(1, half):
            tw[k] = tw[k - 1] * wl % R
        for s in range(0, n, 2 * half):
            for k in range(half):
                u, t = v[s + k], v[s + k + half] * tw[k] % R
                v[s + k], v[s + k + half] = (u + t) % R, (u - t) % R
        half *= 2
    return v


def element(b, mode):
    return int.from_bytes(b, "little" if mode == MODE_CKZG else "big")


def to_bytes(x, mode):
    return x.to_bytes(32, "little" if mode == MODE_CKZG else "big")


def poly_from_blob(blob, mode):
    """the coefficients of the polynomial the blob stands for in `mode` (the proof calls' reading of it)"""
    vals = [element(blob[32 * i:32 * i + 32], mode) for i in range(N_BLOB)]
    if mode == MODE_REFERENCE:
        return [v % R for v in vals]
    assert all(v < R for v in vals), "non-canonical element"
    nat = brp(vals)   # nat[j] = p(w^j)
    inv_n = pow(N_BLOB, R - 2, R)
    return [c * inv_n % R for c in ntt(nat, pow(W4096, R - 2, R))]


def blob_from_poly(coeffs, mode):
    """the blob that stands for `coeffs` in `mode`"""
    if mode == MODE_REFERENCE:
        return b"".join(to_bytes(c, mode) for c in coeffs)
    return b"".join(to_bytes(v, mode) for v in brp(ntt(list(coeffs), W4096)))


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def domain():
    """D[j] = w8192^bitrev13(j): brp(roots(8192))"""
    return brp(roots(N_EXT))


def cell_values(coeffs):
    """the 8192 values p(D[j]) by one 8192-point transform of the zero-padded coefficients"""
    ev = ntt(list(coeffs) + [0] * (N_EXT - len(coeffs)), W8192)
    return brp(ev)


def cells_bytes(coeffs, mode):
    vals = cell_values(coeffs)
    flat = b"".join(to_bytes(v, mode) for v in vals)
    return [flat[2048 * k:2048 * (k + 1)] for k in range(N_CELLS)]


def coset_for_cell(k):
    """the spec's coset_for_cell: w8192^bitrev13(64 k) times the 64th roots of unity, in brp order"""
    shift = pow(W8192, rev(N_CELL * k, 13), R)
    return [shift * r % R for r in brp(roots(N_CELL))]


def c_of_cell(k):
    """c_k = D[64 k]^64 = w128^bitrev7(k): X^64 - c_k vanishes on cell k's coset"""
    return pow(pow(W8192, rev(N_CELL * k, 13), R), N_CELL, R)


def vanishing_polynomialcoeff(xs):
    p = [1]
    for x in xs:
        q = [0] * (len(p) + 1)
        for i, c in enumerate(p):
            q[i] = (q[i] - x * c) % R
            q[i + 1] = (q[i + 1] + c) % R
        p = q
    return p


def divide_polynomialcoeff(a, b):
    """the spec's long division: the quotient of a by b (coefficients low to high)"""
    a = list(a)
    o = []
    apos, bpos = len(a) - 1, len(b) - 1
    diff = apos - bpos
    inv_lead = pow(b[bpos], R - 2, R)
    while diff >= 0:
        quot = a[apos] * inv_lead % R
        o.insert(0, quot)
        for i in range(bpos, -1, -1):
            a[diff + i] = (a[diff + i] - b[i] * quot) % R
        apos -= 1
        diff -= 1
    return [x % R for x in o]


def quotient(coeffs, k):
    """q_k = p div (X^64 - c_k) by the binomial recurrence, 4032 coefficients (degree < 4032)"""
    c = c_of_cell(k)
    n = N_BLOB - N_CELL
    q = [0] * n
    for j in range(n - 1, -1, -1):
        q[j] = (coeffs[j + N_CELL] + (c * q[j + N_CELL] if j + N_CELL < n else 0)) % R
    return q


def remainder(coeffs, k):
    """p mod (X^64 - c_k), 64 coefficients: the interpolant I_k of cell k's values"""
    c = c_of_cell(k)
    out = [0] * N_CELL
    ck = 1
    for m in range(N_BLOB // N_CELL):
        for t in range(N_CELL):
            out[t] = (out[t] + coeffs[N_CELL * m + t] * ck) % R
        ck = ck * c % R
    return out
