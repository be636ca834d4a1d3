"""CPU: the Python restatement of EIP-7594 cells and cell proofs (tests/cells_spec.py) that tests/test_gpu_cells.py checks the library
against, held against the definitions themselves: direct Horner evaluation at sampled points, the spec's long division and its
remainder, the literal coset_for_cell, w8192^2 = the library's w4096, and the c-kzg property that cells 0 .. 63 are the blob. Also the
constant cells.hip scales by, parsed from the source."""
import os
import random
import re

import blobs as B
import cells_spec as S
from conftest import ROOT


def _coeffs(seed):
    rnd = random.Random(seed)
    return [rnd.randrange(S.R) for _ in range(S.N_BLOB)]


def _limbs(name, path):
    src = open(os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc", path)).read()
    m = re.search(name + r"\[8\]\s*=\s*\{([^}]*)\}", src)
    words = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
    return sum(w << (32 * i) for i, w in enumerate(words))


def test_omega8192_squared_is_the_library_omega4096():
    assert pow(S.W8192, 2, S.R) == S.W4096 == _limbs("kOmegaRaw", "fr_ops.hip")
    assert pow(S.W8192, 4096, S.R) == S.R - 1
    # cells.hip: w8192 R^2 mod r, R = 2^256
    assert _limbs("kOmega8192R2", "cells.hip") == S.W8192 * pow(2, 512, S.R) % S.R


def test_coset_for_cell_is_the_literal_slice_of_the_bit_reversed_domain():
    dom = S.domain()
    assert dom == S.brp(S.roots(S.N_EXT))
    for k in (0, 1, 63, 64, 65, 127):
        assert S.coset_for_cell(k) == dom[64 * k:64 * k + 64]
        assert all(pow(x, 64, S.R) == S.c_of_cell(k) for x in S.coset_for_cell(k))
    # c_k = w128^bitrev7(k)
    w128 = pow(7, (S.R - 1) // 128, S.R)
    assert [S.c_of_cell(k) for k in range(128)] == [pow(w128, S.rev(k, 7), S.R) for k in range(128)]
    # the first half of the extended domain is the blob's own (bit-reversed 4096) domain
    assert dom[:4096] == S.brp(S.roots(4096))


def test_cells_by_transform_equal_horner_at_sampled_points():
    p = _coeffs(1)
    vals = S.cell_values(p)
    dom = S.domain()
    rnd = random.Random(2)
    for j in [0, 63, 64, 4095, 4096, 4097, 8191] + [rnd.randrange(8192) for _ in range(8)]:
        assert vals[j] == S.evaluate(p, dom[j]), j


def test_quotient_is_the_spec_long_division_and_leaves_the_remainder():
    p = _coeffs(3)
    for k in (0, 5, 64, 127):
        xs = S.coset_for_cell(k)
        van = S.vanishing_polynomialcoeff(xs)
        assert van == [(-S.c_of_cell(k)) % S.R] + [0] * 63 + [1]
        q = S.quotient(p, k)
        assert q == S.divide_polynomialcoeff(p, van)
        rem = S.remainder(p, k)
        # q (X^64 - c) + rem == p
        prod = [0] * 4096
        for j, c in enumerate(q):
            prod[j + 64] = (prod[j + 64] + c) % S.R
            prod[j] = (prod[j] - S.c_of_cell(k) * c) % S.R
        assert [(a + (rem[i] if i < 64 else 0)) % S.R for i, a in enumerate(prod)] == p
        # the remainder interpolates the cell
        for x in xs[:4]:
            assert S.evaluate(rem, x) == S.evaluate(p, x)


def test_ckzg_cells_0_to_63_are_the_blob_and_the_modes_agree():
    blob_le = B.synthetic_blob(7, big_endian=False)
    p = S.poly_from_blob(blob_le, S.MODE_CKZG)
    cells = S.cells_bytes(p, S.MODE_CKZG)
    assert b"".join(cells[:64]) == blob_le
    assert S.blob_from_poly(p, S.MODE_CKZG) == blob_le
    # the same polynomial in reference mode: every element byte-reversed
    ref = S.cells_bytes(S.poly_from_blob(S.blob_from_poly(p, S.MODE_REFERENCE), S.MODE_REFERENCE), S.MODE_REFERENCE)
    for k in (0, 64, 127):
        assert ref[k] == b"".join(cells[k][32 * t:32 * t + 32][::-1] for t in range(64))
