"""GPU: EIP-7594 recovery (lwkzg_recover_cells_and_kzg_proofs, _batch, _batch_device) in both modes. The expected outputs are
lwkzg_compute_cells_and_kzg_proofs' for the original blob, which tests/test_gpu_cells.py pins to the Python restatement: byte for byte
over ten index patterns (one also against tests/recover_spec.py's coefficients), edge polynomials, batches across the 8-blob launch
set in the three forms, one call across the kernels' group of 256 blobs, outputs left out, the caller's stream, elements not below r and inconsistent cells in the middle of a batch,
exactly 64 cells with an altered element (another polynomial, not an error), the round trip through the cell proof verifier, both
engines, a Lagrange-only table and the other two setups."""
import contextlib
import ctypes as C
import random

import pytest

import blobs as B
import cells_spec as S
import recover_spec as RS
from conftest import R, SETUP_PATH, SETUP_TAU2_PATH, SETUP_UNSTRUCTURED_PATH

pytestmark = pytest.mark.gpu

INF = bytes([0xc0]) + bytes(47)
MODES = [S.MODE_REFERENCE, S.MODE_CKZG]
CELL = 2048


@contextlib.contextmanager
def _mode(K, ts, mode):
    K.lib().lwkzg_settings_set_mode(ts.ref(), mode)
    try:
        yield
    finally:
        K.lib().lwkzg_settings_set_mode(ts.ref(), -1)


def _blob(seed, mode):
    return B.synthetic_blob(seed, big_endian=mode == S.MODE_REFERENCE)


def _pick(count, seed):
    return sorted(random.Random(seed).sample(range(128), count))


def _bad_code(K, mode):
    return K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR


def _given(full_cells, idx):
    """the cells at idx of one blob's 128, concatenated"""
    return b"".join(full_cells[k] for k in idx)


def _alter(cells, i, t, mode, value=None):
    """element t of the i-th given cell replaced (by value, or by itself + 1)"""
    out = bytearray(cells)
    at = CELL * i + 32 * t
    v = (S.element(bytes(out[at:at + 32]), mode) + 1) % R if value is None else value
    out[at:at + 32] = S.to_bytes(v, mode)
    return bytes(out)


def _dev(torch, data):
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


def _device(K, torch, idx, cells, n, ts, cells_out=True, proofs=True, stream=None):
    din = _dev(torch, cells)
    dc = torch.zeros(max(n, 1) * 128 * CELL, dtype=torch.uint8, device="cuda") if cells_out else None
    dp = torch.zeros(max(n, 1) * 128 * 48, dtype=torch.uint8, device="cuda") if proofs else None
    ds = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    K.recover_cells_and_kzg_proofs_batch_device(dc.data_ptr() if cells_out else None, dp.data_ptr() if proofs else None, idx, din.data_ptr(),
                                                n, ts, stream, ds.data_ptr())
    torch.cuda.synchronize()
    cr = bytes(dc.cpu().numpy()) if cells_out else None
    pr = bytes(dp.cpu().numpy()) if proofs else None
    return K.capi._cells_split(cr, pr, n), ds.cpu().tolist()[:n]


PATTERNS = [
    ("cells_0_to_63", list(range(64))),
    ("cells_64_to_127", list(range(64, 128))),
    ("even", list(range(0, 128, 2))),
    ("odd", list(range(1, 128, 2))),
    ("random_64", _pick(64, 1)),
    ("random_65", _pick(65, 2)),
    ("random_100", _pick(100, 3)),
    ("all_but_cell_0", list(range(1, 128))),
    ("all_but_cell_127", list(range(127))),
    ("all_128", list(range(128))),
]


@pytest.mark.parametrize("mode", MODES)
def test_index_patterns(K, gpu_setup, mode):
    with _mode(K, gpu_setup, mode):
        for j, (name, idx) in enumerate(PATTERNS):
            want = K.compute_cells_and_kzg_proofs(_blob(900 + j, mode), gpu_setup)
            got = K.recover_cells_and_kzg_proofs(idx, _given(want[0], idx), gpu_setup)
            assert got[0] == want[0], name
            assert got[1] == want[1], name


@pytest.mark.parametrize("mode", MODES)
def test_against_the_restated_spec(K, gpu_setup, mode):
    idx = _pick(65, 2)
    blob = _blob(930, mode)
    full = S.cells_bytes(S.poly_from_blob(blob, mode), mode)
    values = [[S.element(full[k][32 * t:32 * t + 32], mode) for t in range(64)] for k in idx]
    coeffs = RS.recover_polynomialcoeff(idx, values)
    assert not any(coeffs[4096:])
    with _mode(K, gpu_setup, mode):
        got, _ = K.recover_cells_and_kzg_proofs(idx, _given(full, idx), gpu_setup, proofs=False)
    assert got == S.cells_bytes(coeffs[:4096], mode)


def _edge_blobs(mode):
    rnd = random.Random(99)
    return {
        "zero": (bytes(4096 * 32), "inf"),
        "constant": (S.blob_from_poly([12345] + [0] * 4095, mode), "inf"),
        "x64": (S.blob_from_poly([0] * 64 + [1] + [0] * 4031, mode), "gen"),
        "degree_below_64": (S.blob_from_poly([rnd.randrange(R) for _ in range(64)] + [0] * 4032, mode), "inf"),
        "all_r_minus_1": (S.to_bytes(R - 1, mode) * 4096, None),
    }


@pytest.mark.parametrize("mode", MODES)
def test_edge_polynomials(K, gpu_setup, oracle, mode):
    gen = oracle.g1_generator_mul(1)
    with _mode(K, gpu_setup, mode):
        for j, (name, (blob, kind)) in enumerate(_edge_blobs(mode).items()):
            idx = _pick(64, 40 + j)
            want = K.compute_cells_and_kzg_proofs(blob, gpu_setup)
            got = K.recover_cells_and_kzg_proofs(idx, _given(want[0], idx), gpu_setup)
            assert got == want, name
            if kind == "inf":
                assert got[1] == [INF] * 128, name
            elif kind == "gen":
                assert got[1] == [gen] * 128, name


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 9, 17])
def test_batches_across_the_launch_set(K, gpu_setup, mode, n):
    import torch
    idx = _pick(64, 50 + n)
    with _mode(K, gpu_setup, mode):
        want = K.compute_cells_and_kzg_proofs_batch(b"".join(_blob(1000 + i, mode) for i in range(n)), gpu_setup)
        cells = b"".join(_given(w[0], idx) for w in want)
        assert K.recover_cells_and_kzg_proofs_batch(idx, cells, n, gpu_setup) == want
        got, status = _device(K, torch, idx, cells, n, gpu_setup)
        assert status == [0] * n
        assert got == want
        singles = [K.recover_cells_and_kzg_proofs(idx, cells[64 * CELL * b:64 * CELL * (b + 1)], gpu_setup) for b in range(n)]
        assert singles == want


def test_a_shared_set_call_across_the_kernels_group_of_256_blobs(K, gpu_setup):
    """a chunk without proofs holds up to 512 blobs and reaches the kernels 256 at a time, every blob with set id 0 and its cells
    65 b cells into the input: blob 256, the first of the second group, has an altered element, so its cells are inconsistent. It
    alone is flagged and every other blob's cells are the compute call's. One device call, compared on the device."""
    import torch
    mode = S.MODE_REFERENCE
    n, idx = 257, _pick(65, 150)
    with _mode(K, gpu_setup, mode):
        db = _dev(torch, b"".join(_blob(2000 + i, mode) for i in range(n)))
        want = torch.zeros(n * 128 * CELL, dtype=torch.uint8, device="cuda")
        got = torch.zeros(n * 128 * CELL, dtype=torch.uint8, device="cuda")
        ds = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        K.compute_cells_and_kzg_proofs_batch_device(want.data_ptr(), None, db.data_ptr(), n, gpu_setup)
        torch.cuda.synchronize()
        given = want.view(n, 128, CELL)[:, idx, :].contiguous()
        spoilt = _alter(bytes(given[256, 32].cpu().numpy()), 0, 7, mode)
        given[256, 32] = _dev(torch, spoilt)
        torch.cuda.synchronize()
        K.recover_cells_and_kzg_proofs_batch_device(got.data_ptr(), None, idx, given.data_ptr(), n, gpu_setup, None, ds.data_ptr())
        torch.cuda.synchronize()
        assert ds.cpu().tolist() == [0] * 256 + [_bad_code(K, mode)]
        assert torch.equal(got.view(n, -1)[:256], want.view(n, -1)[:256])


@pytest.mark.parametrize("mode", MODES)
def test_outputs_may_be_left_out_and_calls_repeat(K, gpu_setup, mode):
    import torch
    idx = _pick(70, 60)
    n = 3
    with _mode(K, gpu_setup, mode):
        want = K.compute_cells_and_kzg_proofs_batch(b"".join(_blob(1100 + i, mode) for i in range(n)), gpu_setup)
        cells = b"".join(_given(w[0], idx) for w in want)
        assert K.recover_cells_and_kzg_proofs_batch(idx, cells, n, gpu_setup) == want
        assert K.recover_cells_and_kzg_proofs_batch(idx, cells, n, gpu_setup) == want   # a second call: the same bytes
        assert K.recover_cells_and_kzg_proofs_batch(idx, cells, n, gpu_setup, proofs=False) == [(c, None) for c, _ in want]
        assert K.recover_cells_and_kzg_proofs_batch(idx, cells, n, gpu_setup, cells_out=False) == [(None, p) for _, p in want]
        assert _device(K, torch, idx, cells, n, gpu_setup, proofs=False)[0] == [(c, None) for c, _ in want]
        assert _device(K, torch, idx, cells, n, gpu_setup, cells_out=False)[0] == [(None, p) for _, p in want]
        assert K.recover_cells_and_kzg_proofs(idx, cells[:70 * CELL], gpu_setup, proofs=False) == (want[0][0], None)
        assert K.recover_cells_and_kzg_proofs(idx, cells[:70 * CELL], gpu_setup, cells_out=False) == (None, want[0][1])


def test_empty_calls(K, gpu_setup):
    idx = list(range(64))
    assert K.recover_cells_and_kzg_proofs_batch(idx, b"", 0, gpu_setup) == []
    arr = (C.c_uint64 * 64)(*idx)
    assert K.lib().lwkzg_recover_cells_and_kzg_proofs_batch(None, None, arr, None, 64, 0, gpu_setup.ref(), None) == K.C_KZG_OK
    assert K.lib().lwkzg_recover_cells_and_kzg_proofs_batch_device(None, None, None, None, 0, 0, gpu_setup.ref(), None, None) == K.C_KZG_OK


def test_callers_stream(K, gpu_setup):
    import torch
    idx = _pick(64, 70)
    want = K.compute_cells_and_kzg_proofs_batch(b"".join(_blob(1200 + i, S.MODE_REFERENCE) for i in range(2)), gpu_setup)
    cells = b"".join(_given(w[0], idx) for w in want)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        din = _dev(torch, cells)
        dc = torch.empty(2 * 128 * CELL, dtype=torch.uint8, device="cuda")
        dp = torch.empty(2 * 128 * 48, dtype=torch.uint8, device="cuda")
        K.recover_cells_and_kzg_proofs_batch_device(dc.data_ptr(), dp.data_ptr(), idx, din.data_ptr(), 2, gpu_setup, s.cuda_stream)
        cr, pr = dc.cpu(), dp.cpu()
    s.synchronize()
    assert K.capi._cells_split(bytes(cr.numpy()), bytes(pr.numpy()), 2) == want


def _rejected_in_the_middle(K, torch, ts, mode, idx, want, cells, bad_blob=2):
    """`cells`: 5 blobs' given cells with blob 2 spoilt. The host call fails with the mode's code and writes nothing, the device form
    flags blob 2 alone and the other four are right."""
    n, num = 5, len(idx)
    out_c = C.create_string_buffer(b"\x5a" * (n * 128 * CELL), n * 128 * CELL)
    out_p = C.create_string_buffer(b"\x5a" * (n * 128 * 48), n * 128 * 48)
    first_bad = C.c_size_t(12345)
    arr = (C.c_uint64 * num)(*idx)
    rc = K.lib().lwkzg_recover_cells_and_kzg_proofs_batch(out_c, out_p, arr, cells, num, n, ts.ref(), C.byref(first_bad))
    assert rc == _bad_code(K, mode) and first_bad.value == bad_blob
    assert out_c.raw == b"\x5a" * (n * 128 * CELL) and out_p.raw == b"\x5a" * (n * 128 * 48)   # nothing written
    got, status = _device(K, torch, idx, cells, n, ts)
    assert [s != 0 for s in status] == [i == bad_blob for i in range(n)]
    assert status[bad_blob] == _bad_code(K, mode)
    assert [g for i, g in enumerate(got) if i != bad_blob] == [w for i, w in enumerate(want) if i != bad_blob]


@pytest.mark.parametrize("mode", MODES)
def test_an_element_not_below_r_in_the_middle_of_a_batch(K, gpu_setup, mode):
    """never reduced, not in reference mode either"""
    import torch
    idx = _pick(64, 80)
    with _mode(K, gpu_setup, mode):
        want = K.compute_cells_and_kzg_proofs_batch(b"".join(_blob(1300 + i, mode) for i in range(5)), gpu_setup)
        per = [_given(w[0], idx) for w in want]
        for value in (R, 2 ** 256 - 1):
            spoilt = list(per)
            spoilt[2] = _alter(per[2], 31, 63, mode, value=value)
            _rejected_in_the_middle(K, torch, gpu_setup, mode, idx, want, b"".join(spoilt))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", [65, 128])
def test_inconsistent_cells_in_the_middle_of_a_batch(K, gpu_setup, mode, count):
    import torch
    idx = _pick(count, 90)
    with _mode(K, gpu_setup, mode):
        want = K.compute_cells_and_kzg_proofs_batch(b"".join(_blob(1400 + i, mode) for i in range(5)), gpu_setup)
        per = [_given(w[0], idx) for w in want]
        per[2] = _alter(per[2], count // 2, 7, mode)
        _rejected_in_the_middle(K, torch, gpu_setup, mode, idx, want, b"".join(per))
        # the single form: the mode's code, nothing written
        with pytest.raises(K.KzgError) as e:
            K.recover_cells_and_kzg_proofs(idx, per[2], gpu_setup)
        assert e.value.rc == _bad_code(K, mode)


@pytest.mark.parametrize("mode", MODES)
def test_exactly_64_cells_with_an_altered_element_are_another_polynomial(K, gpu_setup, mode):
    idx = _pick(64, 100)
    with _mode(K, gpu_setup, mode):
        full, _ = K.compute_cells_and_kzg_proofs(_blob(1500, mode), gpu_setup, proofs=False)
        given = _alter(_given(full, idx), 20, 33, mode)
        cells, proofs = K.recover_cells_and_kzg_proofs(idx, given, gpu_setup)
        assert b"".join(cells[k] for k in idx) == given
        # the blob that stands for the recovered polynomial: its evaluations on the 4096 domain are cells 0 .. 63
        evals = b"".join(cells[:64])
        if mode == S.MODE_CKZG:
            blob = evals
        else:
            le = b"".join(evals[32 * i:32 * i + 32][::-1] for i in range(4096))
            blob = S.blob_from_poly(S.poly_from_blob(le, S.MODE_CKZG), S.MODE_REFERENCE)
        assert (cells, proofs) == K.compute_cells_and_kzg_proofs(blob, gpu_setup)
        assert cells != full


@pytest.mark.parametrize("mode", MODES)
def test_recovered_cells_and_proofs_pass_the_verifier(K, gpu_setup, mode):
    idx = _pick(64, 110)
    with _mode(K, gpu_setup, mode):
        blobs = [_blob(1600 + i, mode) for i in range(2)]
        comms = K.blob_to_kzg_commitment_batch(b"".join(blobs), gpu_setup)
        full = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), gpu_setup, proofs=False)
        got = K.recover_cells_and_kzg_proofs_batch(idx, b"".join(_given(f[0], idx) for f in full), 2, gpu_setup)
        items = [(comms[b], k, got[b][0][k], got[b][1][k]) for b in range(2) for k in range(128)]
        cols = list(zip(*items))
        assert K.verify_cell_kzg_proof_batch(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), gpu_setup) is True
        swapped = list(cols[3])
        swapped[5], swapped[6] = swapped[6], swapped[5]
        assert K.verify_cell_kzg_proof_batch(list(cols[0]), list(cols[1]), list(cols[2]), swapped, gpu_setup) is False


@pytest.mark.parametrize("mode", MODES)
def test_both_engines(K, engine_setup, mode):
    idx = _pick(64, 120)
    with _mode(K, engine_setup, mode):
        want = K.compute_cells_and_kzg_proofs(_blob(1700, mode), engine_setup)
        assert K.recover_cells_and_kzg_proofs(idx, _given(want[0], idx), engine_setup) == want


def test_lagrange_only_table_in_ckzg_mode(K):
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        ts.set_mode(K.MODE_CKZG)
        ts.enable_direct_table_forms(10, 2)
        assert ts.direct_table_forms() == 2
        idx = _pick(64, 130)
        want = K.compute_cells_and_kzg_proofs(_blob(1800, S.MODE_CKZG), ts)
        assert K.recover_cells_and_kzg_proofs(idx, _given(want[0], idx), ts) == want
    finally:
        ts.free()


@pytest.mark.parametrize("path", [SETUP_TAU2_PATH, SETUP_UNSTRUCTURED_PATH], ids=["tau2", "unstructured"])
@pytest.mark.parametrize("mode", MODES)
def test_the_second_and_the_unstructured_setup(K, gpu_setup, mode, path):
    idx = _pick(64, 140)
    ts = K.TrustedSetup.from_file(path)
    try:
        with _mode(K, ts, mode):
            want = K.compute_cells_and_kzg_proofs(_blob(1900, mode), ts)
            assert K.recover_cells_and_kzg_proofs(idx, _given(want[0], idx), ts) == want
    finally:
        ts.free()
