"""CPU: the Python restatement of EIP-7594 verify_cell_kzg_proof_batch (tests/cell_verify_spec.py) that tests/test_gpu_cell_verify.py
checks the library against, held against the definitions themselves -- both interpolation routes equal p mod (X^64 - c_k), the
per-item identity holds for honest items and fails for an altered one -- and what the library decides without a GPU: the two-level
transcript (lwkzg_cell_batch_challenge_host) against hashlib in both modes, the argument checks, and the constants
cells_verify.hip scales by, parsed from the source."""
import ctypes as C
import os
import random
import re

import cell_verify_spec as V
import cells_spec as S
from conftest import ROOT, TAU, tau_closed_form

MODES = [S.MODE_REFERENCE, S.MODE_CKZG]


def _coeffs(seed):
    rnd = random.Random(seed)
    return [rnd.randrange(S.R) for _ in range(S.N_BLOB)]


def _honest_items(oracle, seed, ks, mode):
    p = _coeffs(seed)
    cells = S.cells_bytes(p, mode)
    cm = tau_closed_form(oracle, p)
    return [(cm, k, cells[k], tau_closed_form(oracle, S.quotient(p, k))) for k in ks]


def test_both_interpolation_routes_give_the_remainder():
    p = _coeffs(11)
    vals = S.cell_values(p)
    for k in (0, 1, 64, 77, 127):
        want = S.remainder(p, k)
        cell = vals[64 * k:64 * k + 64]
        assert V.interpolant_by_transform(cell, k) == want, k
        if k in (0, 64, 127):
            assert V.interpolant(cell, k) == want, k


def test_per_item_identity_holds_for_honest_items_and_fails_for_an_altered_element(oracle):
    for mode in MODES:
        items = _honest_items(oracle, 21 + mode, (0, 64, 127), mode)
        for it in items:
            assert V.item_holds_known_tau(oracle, it, mode, TAU)
        c, k, cell, proof = items[1]
        t = 17
        v = (S.element(cell[32 * t:32 * t + 32], mode) + 1) % S.R
        altered = cell[:32 * t] + S.to_bytes(v, mode) + cell[32 * t + 32:]
        assert not V.item_holds_known_tau(oracle, (c, k, altered, proof), mode, TAU)
        assert not V.item_holds_known_tau(oracle, (c, 65, cell, proof), mode, TAU)
        assert V.verdict_known_tau(oracle, items, mode, TAU)
        assert not V.verdict_known_tau(oracle, [items[0], (c, k, altered, proof), items[2]], mode, TAU)


def _random_items(seed, commitments, ks):
    rnd = random.Random(seed)
    return [(commitments[j], k, bytes(rnd.getrandbits(8) for _ in range(2048)), bytes(rnd.getrandbits(8) for _ in range(48))) for j, k in ks]


def test_challenge_host_matches_the_restatement(K):
    from lambdaworks_kzg_amd import capi
    rnd = random.Random(5)
    cms = [bytes(rnd.getrandbits(8) for _ in range(48)) for _ in range(3)]
    cases = [_random_items(1, cms, [(0, 5)]),
             _random_items(2, cms, [(0, 0), (1, 127), (0, 64), (2, 3), (1, 127)]),   # repeated commitments, interleaved
             []]
    for items in cases:
        for mode in MODES:
            got = capi.cell_batch_challenge_host([it[0] for it in items], [it[1] for it in items], [it[2] for it in items],
                                                 [it[3] for it in items], mode)
            assert got == S.to_bytes(V.challenge(items, mode), mode), (len(items), mode)
    # the transcript tells rows apart: the same items under another commitment pattern give another r
    a = _random_items(2, cms, [(0, 0), (1, 1)])
    b = [(cms[0],) + a[0][1:], (cms[0],) + a[1][1:]]
    assert V.challenge(a, 0) != V.challenge(b, 0)


def test_argument_checks_need_no_gpu(K):
    from lambdaworks_kzg_amd import capi
    l = K.lib()
    s = K.KZGSettings()
    ok = C.c_bool(True)
    cm, cell, pf = bytes(48), bytes(2048), bytes(48)
    one = (C.c_uint64 * 1)(3)
    # the empty batch answers true without touching anything
    assert l.lwkzg_verify_cell_kzg_proof_batch(C.byref(ok), None, None, None, None, 0, C.byref(s)) == K.C_KZG_OK and ok.value is True
    for args in [(None, one, cell, pf), (cm, None, cell, pf), (cm, one, None, pf), (cm, one, cell, None)]:
        ok.value = True
        assert l.lwkzg_verify_cell_kzg_proof_batch(C.byref(ok), *args, 1, C.byref(s)) == K.C_KZG_BADARGS
        assert ok.value is False
    assert l.lwkzg_verify_cell_kzg_proof_batch(None, cm, one, cell, pf, 1, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_verify_cell_kzg_proof_batch(C.byref(ok), cm, one, cell, pf, 1, None) == K.C_KZG_BADARGS
    # an index of 128 or more is decided before any device work
    for k in (128, 129, 2 ** 63, 2 ** 64 - 1):
        idx = (C.c_uint64 * 2)(5, k)
        ok.value = True
        assert l.lwkzg_verify_cell_kzg_proof_batch(C.byref(ok), cm * 2, idx, cell * 2, pf * 2, 2, C.byref(s)) == K.C_KZG_BADARGS, k
        assert ok.value is False
        out = C.create_string_buffer(capi.CELL_VERIFY_PARTIAL_BYTES)
        assert l.lwkzg_cell_verify_partials(out, cm * 2, idx, cell * 2, pf * 2, 2, C.byref(s)) == K.C_KZG_BADARGS
        r = C.create_string_buffer(32)
        assert l.lwkzg_cell_batch_challenge_host(r, cm * 2, idx, cell * 2, pf * 2, 2, 0) == K.C_KZG_BADARGS
    r = C.create_string_buffer(32)
    assert l.lwkzg_cell_batch_challenge_host(r, cm, one, cell, pf, 1, 7) == K.C_KZG_BADARGS       # no such mode
    assert l.lwkzg_cell_batch_challenge_host(None, cm, one, cell, pf, 1, 0) == K.C_KZG_BADARGS
    assert l.lwkzg_cell_batch_challenge_host(r, None, one, cell, pf, 1, 0) == K.C_KZG_BADARGS
    assert l.lwkzg_cell_verify_partials(None, cm, one, cell, pf, 1, C.byref(s)) == K.C_KZG_BADARGS


def _limbs(name):
    src = open(os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc", "recover_consts.inc")).read()
    m = re.search(name + r"\[8\]\s*=\s*\{([^}]*)\}", src)
    words = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
    return sum(w << (32 * i) for i, w in enumerate(words))


def test_kernel_constants():
    mont = pow(2, 256, S.R)
    assert _limbs("kRecInvOmega8192Mont") == pow(S.W8192, S.R - 2, S.R) * mont % S.R
    assert _limbs("kRecInv64Mont") == pow(64, S.R - 2, S.R) * mont % S.R
    # what k_cellv_columns relies on: D[64 k] = w8192^bitrev7(k), and the inverse twiddle of exponent e is -w4096^-(e - 2048) above 2048
    for k in (0, 1, 64, 77, 127):
        assert S.coset_for_cell(k)[0] == pow(S.W8192, S.rev(k, 7), S.R)
    assert pow(S.W4096, 2048, S.R) == S.R - 1
