"""CPU: EIP-7594 recovery. The two Python routes of tests/recover_spec.py (the consensus-specs 8192-point algorithm and the factored
one csrc/recover.hip runs) against each other and against the polynomial they started from, the consistency criterion, the constants
baked into the kernels against Python's pow, and the argument checks of the three entry points, which need no GPU."""
import ctypes as C
import functools
import os
import random
import re

import cells_spec as S
import recover_spec as RS
from conftest import ROOT

R = S.R


@functools.lru_cache(maxsize=None)
def _poly():
    rnd = random.Random(7594)
    coeffs = [rnd.randrange(R) for _ in range(S.N_BLOB)]
    vals = S.cell_values(coeffs)
    return coeffs, [vals[64 * k:64 * k + 64] for k in range(S.N_CELLS)]


def _pick(count, seed):
    return sorted(random.Random(seed).sample(range(S.N_CELLS), count))


def test_both_routes_return_the_polynomial():
    coeffs, cells = _poly()
    for count in (64, 70):
        idx = _pick(count, count)
        given = [cells[k] for k in idx]
        full = RS.recover_polynomialcoeff(idx, given)
        assert full[:S.N_BLOB] == coeffs and not any(full[S.N_BLOB:]), count
        got, upper = RS.recover_factored(idx, given)
        assert got == coeffs, count
        assert not any(any(u) for u in upper), count


def test_an_altered_element_among_70_cells_is_inconsistent_on_both_routes():
    coeffs, cells = _poly()
    idx = _pick(70, 70)
    given = [list(cells[k]) for k in idx]
    given[33][17] = (given[33][17] + 1) % R
    full = RS.recover_polynomialcoeff(idx, given)
    assert any(full[S.N_BLOB:])
    _, upper = RS.recover_factored(idx, given)
    # element 17 of a cell enters every I_k[t]: all 64 decodings see it
    assert any(any(u) for u in upper)


def test_an_altered_element_among_exactly_64_cells_is_another_polynomial():
    coeffs, cells = _poly()
    idx = _pick(64, 64)
    given = [list(cells[k]) for k in idx]
    given[5][40] = (given[5][40] + 12345) % R
    got, upper = RS.recover_factored(idx, given)
    assert not any(any(u) for u in upper)
    assert got != coeffs
    vals = S.cell_values(got)
    for k, want in zip(idx, given):
        assert vals[64 * k:64 * k + 64] == want, k
    full = RS.recover_polynomialcoeff(idx, given)
    assert full[:S.N_BLOB] == got and not any(full[S.N_BLOB:])


def test_the_interpolant_of_a_cell_is_the_remainder():
    coeffs, cells = _poly()
    for k in (0, 1, 77, 127):
        assert RS.cell_interpolant(k, cells[k]) == S.remainder(coeffs, k), k
    # I_k[t] = P_t(c_k), P_t the polynomial of coefficients 64 m + t
    k, t = 77, 9
    assert S.remainder(coeffs, k)[t] == S.evaluate(coeffs[t::64], S.c_of_cell(k))


def _consts():
    src = open(os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc", "recover_consts.inc")).read()
    out = {}
    for name, body in re.findall(r"(kRec\w+)\[8\]\s*=\s*\{([^}]*)\}", src):
        words = [int(x.strip().rstrip("u"), 16) for x in body.split(",")]
        out[name] = sum(w << (32 * i) for i, w in enumerate(words))
    return out


def test_kernel_constants():
    mont = pow(2, 256, R)
    c = _consts()
    assert c == {
        "kRecGenMont": RS.GEN * mont % R,
        "kRecInvGenMont": pow(RS.GEN, R - 2, R) * mont % R,
        "kRecInv128Mont": pow(128, R - 2, R) * mont % R,
        "kRecInv64Mont": pow(64, R - 2, R) * mont % R,
        "kRecInvOmega8192Mont": pow(S.W8192, R - 2, R) * mont % R,
    }
    # what the kernels rely on: w128 = w4096^32 (entry 32 j of the twiddle tables is w128^j), w128^64 = -1, c_k = w128^bitrev7(k),
    # and 7 times a 128th root of unity is none (the coset's values of Zs can be inverted)
    assert RS.W128 == pow(S.W4096, 32, R) and pow(RS.W128, 64, R) == R - 1
    assert all(S.c_of_cell(k) == pow(RS.W128, S.rev(k, 7), R) for k in range(128))
    assert pow(RS.GEN, 128, R) != 1
    # the committed file is what the generator prints
    import subprocess
    import sys
    gen = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_recover_consts.py")]).decode()
    assert gen == open(os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc", "recover_consts.inc")).read()


def test_argument_checks_need_no_gpu(K):
    l = K.lib()
    s = K.KZGSettings()
    ps = C.byref(s)
    cells_out, proofs = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48)
    first_bad = C.c_size_t(77)

    def arr(v):
        return (C.c_uint64 * max(len(v), 1))(*v)

    def calls(idx, num, out=(cells_out, proofs), cells=True, settings=ps):
        """the three entry points on one blob's worth of arguments"""
        ce = bytes(max(num, 1) * 2048) if cells else None
        a = arr(idx) if idx is not None else None
        return [l.lwkzg_recover_cells_and_kzg_proofs(out[0], out[1], a, ce, num, settings),
                l.lwkzg_recover_cells_and_kzg_proofs_batch(out[0], out[1], a, ce, num, 1, settings, C.byref(first_bad)),
                l.lwkzg_recover_cells_and_kzg_proofs_batch_device(C.cast(out[0], C.c_void_p), C.cast(out[1], C.c_void_p), a,
                                                                  C.cast(C.c_char_p(ce), C.c_void_p) if cells else None, num, 1, settings, None,
                                                                  None)]

    good = list(range(64))
    # n == 0 answers OK without touching anything, whatever else is passed
    assert l.lwkzg_recover_cells_and_kzg_proofs_batch(None, None, None, None, 0, 0, ps, None) == K.C_KZG_OK
    assert l.lwkzg_recover_cells_and_kzg_proofs_batch_device(None, None, None, None, 0, 0, ps, None, None) == K.C_KZG_OK
    assert l.lwkzg_recover_cells_and_kzg_proofs_batch(None, None, None, None, 64, 0, None, None) == K.C_KZG_BADARGS
    bad = [K.C_KZG_BADARGS] * 3
    assert calls(good, 64, settings=None) == bad
    assert calls(None, 64) == bad
    assert calls(good, 64, cells=False) == bad
    assert calls(good, 64, out=(None, None)) == bad
    for num in (0, 63, 129):
        assert calls(list(range(max(num, 1))), num) == bad, num
    for k in (128, 2 ** 64 - 1):
        assert calls(good[:63] + [k], 64) == bad, k
    assert calls(good[:10] + [9] + good[11:], 64) == bad          # a repeated index
    assert calls(good[:10] + [11, 10] + good[12:], 64) == bad     # a descending pair
    assert calls(list(range(1, 65))[::-1], 64) == bad
    assert first_bad.value == 77 and cells_out.raw == bytes(128 * 2048) and proofs.raw == bytes(128 * 48)
    # in c-kzg mode the same code
    prev = K.set_mode(K.MODE_CKZG)
    try:
        assert calls(good, 63) == bad and calls(good[:63] + [128], 64) == bad
    finally:
        K.set_mode(prev)
