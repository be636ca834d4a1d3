"""GPU: EIP-7594 cells and cell proofs (lwkzg_compute_cells_and_kzg_proofs, _batch, _batch_device) in both modes against the Python
restatement of tests/cells_spec.py: cells byte for byte; proofs against the closed form [q_k(tau)]G1 on the tau = 1337 and tau2 setups and
against the unstructured setup's closed form; edge blobs; a non-canonical element in the middle of a batch; cross-checks with
compute_kzg_proof's y, between the modes, and by the pairing e(pi_k, [tau^64 - c_k]G2) e([I_k(tau) - p(tau)]G1, G2) == 1; the three forms,
NULL outputs, batches across the 1024-MSM launch set, n = 0, the caller's stream, both engines and a Lagrange-only table."""
import contextlib
import ctypes as C
import os
import random

import pytest

import blobs as B
import cells_spec as S
import make_setups as M
from conftest import R, SETUP_PATH, SETUP_TAU2_PATH, SETUP_UNSTRUCTURED_PATH, TAU, tau_closed_form, unstructured_closed_form

pytestmark = pytest.mark.gpu

INF = bytes([0xc0]) + bytes(47)
MODES = [S.MODE_REFERENCE, S.MODE_CKZG]


@contextlib.contextmanager
def _mode(K, ts, mode):
    K.lib().lwkzg_settings_set_mode(ts.ref(), mode)
    try:
        yield
    finally:
        K.lib().lwkzg_settings_set_mode(ts.ref(), -1)


def _blob(seed, mode):
    return B.synthetic_blob(seed, big_endian=mode == S.MODE_REFERENCE)


def _want_cells(blob, mode):
    return S.cells_bytes(S.poly_from_blob(blob, mode), mode)


def _want_proofs(oracle, blob, mode, closed=lambda o, q: tau_closed_form(o, q)):
    p = S.poly_from_blob(blob, mode)
    return [closed(oracle, S.quotient(p, k)) for k in range(128)]


def _dev(torch, data):
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


def _device(K, torch, blobs, ts, cells=True, proofs=True, stream=None):
    n = len(blobs) // K.BYTES_PER_BLOB
    db = _dev(torch, blobs)
    dc = torch.zeros(max(n, 1) * 128 * 2048, dtype=torch.uint8, device="cuda") if cells else None
    dp = torch.zeros(max(n, 1) * 128 * 48, dtype=torch.uint8, device="cuda") if proofs else None
    ds = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    K.compute_cells_and_kzg_proofs_batch_device(dc.data_ptr() if cells else None, dp.data_ptr() if proofs else None, db.data_ptr(), n, ts,
                                                stream, ds.data_ptr())
    torch.cuda.synchronize()
    cr = bytes(dc.cpu().numpy()) if cells else None
    pr = bytes(dp.cpu().numpy()) if proofs else None
    return K.capi._cells_split(cr, pr, n), ds.cpu().tolist()[:n]


@pytest.mark.parametrize("mode", MODES)
def test_cells_and_proofs_match_the_restatement(K, gpu_setup, oracle, mode):
    blobs = [_blob(700 + i, mode) for i in range(2)]
    with _mode(K, gpu_setup, mode):
        got = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), gpu_setup)
    for b, (cells, proofs) in zip(blobs, got):
        assert cells == _want_cells(b, mode)
        assert proofs == _want_proofs(oracle, b, mode)


@pytest.mark.parametrize("mode", MODES)
def test_proofs_on_the_second_and_the_unstructured_setup(K, gpu_setup, oracle, mode):
    blob = _blob(710, mode)
    cases = [(SETUP_TAU2_PATH, lambda o, q: tau_closed_form(o, q, tau=M.TAU2)),
             (SETUP_UNSTRUCTURED_PATH, unstructured_closed_form)]
    for path, closed in cases:
        ts = K.TrustedSetup.from_file(path)
        try:
            with _mode(K, ts, mode):
                cells, proofs = K.compute_cells_and_kzg_proofs(blob, ts)
            assert cells == _want_cells(blob, mode), path
            assert proofs == _want_proofs(oracle, blob, mode, closed), path
        finally:
            ts.free()


def _edge_blobs(mode):
    rnd = random.Random(99)
    out = {
        "zero": (bytes(K_BLOB), "inf"),
        "constant": (S.blob_from_poly([12345] + [0] * 4095, mode), "inf"),
        "degree_below_64": (S.blob_from_poly([rnd.randrange(R) for _ in range(64)] + [0] * 4032, mode), "inf"),
        "x64": (S.blob_from_poly([0] * 64 + [1] + [0] * 4031, mode), "gen"),
        "all_r_minus_1": (S.to_bytes(R - 1, mode) * 4096, None),
    }
    if mode == S.MODE_REFERENCE:
        vals = [rnd.randrange(R, 2 ** 256) if i % 3 == 0 else rnd.randrange(R) for i in range(4096)]
        out["elements_at_least_r"] = (b"".join(v.to_bytes(32, "big") for v in vals), None)
    return out


K_BLOB = 4096 * 32


@pytest.mark.parametrize("mode", MODES)
def test_edge_blobs(K, gpu_setup, oracle, mode):
    gen = oracle.g1_generator_mul(1)
    for name, (blob, kind) in _edge_blobs(mode).items():
        with _mode(K, gpu_setup, mode):
            cells, proofs = K.compute_cells_and_kzg_proofs(blob, gpu_setup)
        assert cells == _want_cells(blob, mode), name
        if kind == "inf":
            assert proofs == [INF] * 128, name
        elif kind == "gen":
            assert proofs == [gen] * 128, name
        else:
            assert proofs == _want_proofs(oracle, blob, mode), name
    if mode == S.MODE_REFERENCE:   # elements >= r are reduced: the same outputs as the reduced blob
        blob = _edge_blobs(mode)["elements_at_least_r"][0]
        reduced = b"".join((int.from_bytes(blob[32 * i:32 * i + 32], "big") % R).to_bytes(32, "big") for i in range(4096))
        with _mode(K, gpu_setup, mode):
            assert K.compute_cells_and_kzg_proofs(blob, gpu_setup) == K.compute_cells_and_kzg_proofs(reduced, gpu_setup)


def test_noncanonical_element_in_the_middle_of_a_ckzg_batch(K, gpu_setup):
    import torch
    blobs = [_blob(720 + i, S.MODE_CKZG) for i in range(5)]
    bad = bytearray(blobs[2])
    bad[32 * 100:32 * 101] = R.to_bytes(32, "little")
    blobs[2] = bytes(bad)
    data = b"".join(blobs)
    with _mode(K, gpu_setup, S.MODE_CKZG):
        cells = C.create_string_buffer(5 * 128 * 2048)
        proofs = C.create_string_buffer(5 * 128 * 48)
        first_bad = C.c_size_t(12345)
        rc = K.lib().lwkzg_compute_cells_and_kzg_proofs_batch(cells, proofs, data, 5, gpu_setup.ref(), C.byref(first_bad))
        assert rc == K.C_KZG_BADARGS and first_bad.value == 2
        assert cells.raw == bytes(len(cells.raw))   # nothing written
        singles = [K.compute_cells_and_kzg_proofs(b, gpu_setup) for i, b in enumerate(blobs) if i != 2]
        got, status = _device(K, torch, data, gpu_setup)
    assert [s != 0 for s in status] == [False, False, True, False, False]
    assert [g for i, g in enumerate(got) if i != 2] == singles


@pytest.mark.parametrize("mode", MODES)
def test_cell_values_are_compute_kzg_proof_ys(K, gpu_setup, mode):
    blob = _blob(730, mode)
    dom = S.domain()
    with _mode(K, gpu_setup, mode):
        cells, _ = K.compute_cells_and_kzg_proofs(blob, gpu_setup, proofs=False)
        for k, t in [(0, 0), (3, 17), (63, 63), (64, 0), (100, 5), (127, 63)]:
            _, y = K.compute_kzg_proof(blob, S.to_bytes(dom[64 * k + t], mode), gpu_setup)
            assert cells[k][32 * t:32 * t + 32] == y, (k, t)


def test_reference_blob_and_its_ckzg_form_agree(K, gpu_setup):
    blob_le = _blob(740, S.MODE_CKZG)
    blob_be = S.blob_from_poly(S.poly_from_blob(blob_le, S.MODE_CKZG), S.MODE_REFERENCE)
    with _mode(K, gpu_setup, S.MODE_CKZG):
        c_le, p_le = K.compute_cells_and_kzg_proofs(blob_le, gpu_setup)
    with _mode(K, gpu_setup, S.MODE_REFERENCE):
        c_be, p_be = K.compute_cells_and_kzg_proofs(blob_be, gpu_setup)
    assert p_le == p_be
    for a, b in zip(c_le, c_be):
        assert a == b"".join(b[32 * t:32 * t + 32][::-1] for t in range(64))
    assert b"".join(c_le[:64]) == blob_le


def _g2_lines(path):
    lines = open(path).read().split()
    n1, n2 = int(lines[0]), int(lines[1])
    return [bytes.fromhex(x) for x in lines[2 + n1:2 + n1 + n2]]


@pytest.mark.parametrize("mode", MODES)
def test_cell_proofs_pass_the_pairing_check(K, gpu_setup, oracle, mode):
    g2 = _g2_lines(SETUP_PATH)
    assert M.g2_compress(M.g2_mul_generator(pow(TAU, 64, R))) == g2[64]
    blob = _blob(750, mode)
    p = S.poly_from_blob(blob, mode)
    with _mode(K, gpu_setup, mode):
        _, proofs = K.compute_cells_and_kzg_proofs(blob, gpu_setup)
    p_tau = S.evaluate(p, TAU)
    for k in (0, 77, 127):
        lhs_g2 = M.g2_compress(M.g2_mul_generator((pow(TAU, 64, R) - S.c_of_cell(k)) % R))
        i_g1 = oracle.g1_generator_mul((S.evaluate(S.remainder(p, k), TAU) - p_tau) % R)
        assert K.capi.pairing_product_is_one(proofs[k] + i_g1, lhs_g2 + g2[0]), k
        assert not K.capi.pairing_product_is_one(proofs[(k + 1) % 128] + i_g1, lhs_g2 + g2[0]), k


@pytest.mark.parametrize("mode", MODES)
def test_forms_agree_and_outputs_may_be_left_out(K, gpu_setup, mode):
    import torch
    blobs = [_blob(760 + i, mode) for i in range(3)]
    data = b"".join(blobs)
    with _mode(K, gpu_setup, mode):
        singles = [K.compute_cells_and_kzg_proofs(b, gpu_setup) for b in blobs]
        assert K.compute_cells_and_kzg_proofs_batch(data, gpu_setup) == singles
        assert K.compute_cells_and_kzg_proofs_batch(data, gpu_setup) == singles   # a second call: the same bytes
        got, status = _device(K, torch, data, gpu_setup)
        assert got == singles and status == [0, 0, 0]
        assert K.compute_cells_and_kzg_proofs_batch(data, gpu_setup, proofs=False) == [(c, None) for c, _ in singles]
        assert K.compute_cells_and_kzg_proofs_batch(data, gpu_setup, cells=False) == [(None, p) for _, p in singles]
        assert _device(K, torch, data, gpu_setup, proofs=False)[0] == [(c, None) for c, _ in singles]
        assert _device(K, torch, data, gpu_setup, cells=False)[0] == [(None, p) for _, p in singles]
        assert K.lib().lwkzg_compute_cells_and_kzg_proofs(None, None, blobs[0], gpu_setup.ref()) != K.C_KZG_OK


@pytest.mark.parametrize("n", [9, 17])
def test_batches_across_the_launch_set(K, gpu_setup, n):
    import torch
    mode = S.MODE_CKZG if n == 9 else S.MODE_REFERENCE
    blobs = [_blob(800 + i, mode) for i in range(n)]
    with _mode(K, gpu_setup, mode):
        singles = [K.compute_cells_and_kzg_proofs(b, gpu_setup) for b in blobs]
        got, status = _device(K, torch, b"".join(blobs), gpu_setup)
        assert K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), gpu_setup) == singles
    assert status == [0] * n
    assert got == singles
    assert singles[-1][0] == _want_cells(blobs[-1], mode)


def test_empty_calls(K, gpu_setup):
    assert K.compute_cells_and_kzg_proofs_batch(b"", gpu_setup) == []
    assert K.lib().lwkzg_compute_cells_and_kzg_proofs_batch(None, None, None, 0, gpu_setup.ref(), None) == K.C_KZG_OK
    assert K.lib().lwkzg_compute_cells_and_kzg_proofs_batch_device(None, None, None, 0, gpu_setup.ref(), None, None) == K.C_KZG_OK


def test_callers_stream(K, gpu_setup):
    import torch
    blobs = [_blob(820 + i, S.MODE_REFERENCE) for i in range(2)]
    want = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), gpu_setup)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        db = _dev(torch, b"".join(blobs))
        dc = torch.empty(2 * 128 * 2048, dtype=torch.uint8, device="cuda")
        dp = torch.empty(2 * 128 * 48, dtype=torch.uint8, device="cuda")
        K.compute_cells_and_kzg_proofs_batch_device(dc.data_ptr(), dp.data_ptr(), db.data_ptr(), 2, gpu_setup, s.cuda_stream)
        cr, pr = dc.cpu(), dp.cpu()
    s.synchronize()
    assert K.capi._cells_split(bytes(cr.numpy()), bytes(pr.numpy()), 2) == want


@pytest.mark.parametrize("mode", MODES)
def test_both_engines(K, engine_setup, oracle, mode):
    blob = _blob(840, mode)
    with _mode(K, engine_setup, mode):
        cells, proofs = K.compute_cells_and_kzg_proofs(blob, engine_setup)
    assert cells == _want_cells(blob, mode)
    assert proofs == _want_proofs(oracle, blob, mode)


def test_lagrange_only_table_in_ckzg_mode(K, oracle):
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        ts.set_mode(K.MODE_CKZG)
        ts.enable_direct_table_forms(10, 2)
        assert ts.direct_table_forms() == 2
        blobs = [_blob(850 + i, S.MODE_CKZG) for i in range(2)]
        got = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), ts)
        for b, (cells, proofs) in zip(blobs, got):
            assert cells == _want_cells(b, S.MODE_CKZG)
            assert proofs == _want_proofs(oracle, b, S.MODE_CKZG)
    finally:
        ts.free()
