"""GPU: the column calls (lwkzg_compute_cells_and_kzg_proofs_columns, lwkzg_recover_cells_and_kzg_proofs_columns and their device
forms). The full call is the definition: entry b c + i of a column call is entry 128 b + columns[i] of the full
call on the same blobs and settings, byte for byte. Every batch here is drawn cyclically from 17 distinct blobs, so ONE full call of
17 blobs per mode and settings object is the reference for every shape, sliced; tests/cells_spec.py and the closed form anchor a few
columns on their own. Column sets in all three modes, the slot counts the cells pipeline never produced, one blob past every chunk of
the plan, the host forms across the plan's slice, rejected blobs, the recovery, the engines, FK20 on both sides of its rule, streams."""
import contextlib
import ctypes as C
import random

import pytest

import blobs as B
import cells_spec as S
import make_setups as M
from conftest import R, SETUP_PATH, SETUP_TAU2_PATH, SETUP_UNSTRUCTURED_PATH, tau_closed_form, unstructured_closed_form

pytestmark = pytest.mark.gpu

ETH = 2
MODES = [S.MODE_REFERENCE, S.MODE_CKZG, ETH]
CELL, DISTINCT = 2048, 17
EVEN, ODD, ALL = list(range(0, 128, 2)), list(range(1, 128, 2)), list(range(128))
RANDOM8 = sorted(random.Random(4).sample(range(128), 8))
NEW_KERNELS = ["k_cells_extend_out_columns", "k_cells_quotients_columns", "k_fk20_columns_compress"]
_full_cache = {}


@contextlib.contextmanager
def _mode(K, ts, mode):
    K.lib().lwkzg_settings_set_mode(ts.ref(), mode)
    try:
        yield
    finally:
        K.lib().lwkzg_settings_set_mode(ts.ref(), -1)


def _blob(i, mode):
    """distinct blob i: big-endian canonical elements (coefficients in reference mode, evaluations in eth mode), little-endian in c-kzg mode"""
    return B.synthetic_blob(91000 + i, big_endian=mode != S.MODE_CKZG)


def _blobs(n, mode, first=0):
    return b"".join(_blob((first + b) % DISTINCT, mode) for b in range(n))


def _dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


def _full(K, ts, mode, key="default"):
    """the full call's 128 cells and 128 proofs of the 17 distinct blobs on ts in `mode` (mode set by the caller): made once, never changed"""
    if (key, mode) not in _full_cache:
        _full_cache[(key, mode)] = K.compute_cells_and_kzg_proofs_batch(_blobs(DISTINCT, mode), ts)
    return _full_cache[(key, mode)]


def _want(full, n, cols, first=0):
    """(cells, proofs) bytes of a column call on _blobs(n, mode, first)"""
    cells = b"".join(full[(first + b) % DISTINCT][0][k] for b in range(n) for k in cols)
    proofs = b"".join(full[(first + b) % DISTINCT][1][k] for b in range(n) for k in cols)
    return cells, proofs


def _columns(K, torch, data, n, cols, ts, cells=True, proofs=True, stream=None):
    """the device form on n blobs: (cells bytes or None, proofs bytes or None, status words); outputs pre-filled so that a gap shows"""
    c = len(cols)
    db = _dev(torch, data)
    dc = torch.full((n * c * CELL,), 0x5a, dtype=torch.uint8, device="cuda") if cells else None
    dp = torch.full((n * c * 48,), 0x5a, dtype=torch.uint8, device="cuda") if proofs else None
    ds = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    K.compute_cells_and_kzg_proofs_columns_device(dc.data_ptr() if cells else None, dp.data_ptr() if proofs else None, db.data_ptr(), n, cols, ts,
                                                  stream, ds.data_ptr())
    torch.cuda.synchronize()
    return _host(dc) if cells else None, _host(dp) if proofs else None, ds.cpu().tolist()


def _check(K, torch, ts, full, mode, n, cols, cells=True, proofs=True, first=0):
    want_c, want_p = _want(full, n, cols, first)
    got_c, got_p, status = _columns(K, torch, _blobs(n, mode, first), n, cols, ts, cells, proofs)
    assert status == [0] * n, (n, cols)
    assert got_c == (want_c if cells else None), ("cells", n, cols)
    assert got_p == (want_p if proofs else None), ("proofs", n, cols)


# the plan (cells_columns_plan.h), restated: blobs per chunk on the MSM path and per slice of the host forms
def _chunk(c, cells, proofs=True, recover=False):
    if not proofs:
        return 512
    return min(1024 // c, 512 if cells or recover else 1024)


def _slice(chunk, bytes_per_blob, n):
    chunks = max((64 << 20) // (chunk * bytes_per_blob), 1)
    if chunks * chunk < 64:
        chunks = -(-64 // chunk)
    return min(n, chunks * chunk)


# ---------------------------------------------------------------------------------------------------------------- column sets

@pytest.mark.parametrize("mode", MODES)
def test_a_few_columns_against_the_restatement_and_the_closed_form(K, gpu_setup, oracle, mode):
    cols = [0, 63, 64, 77, 127]
    blob = _blob(0, mode)
    with _mode(K, gpu_setup, mode):
        (cells, proofs), = K.compute_cells_and_kzg_proofs_columns(blob, cols, gpu_setup)
        full = _full(K, gpu_setup, mode)
    poly = S.poly_from_blob(blob, mode)
    want_cells = S.cells_bytes(poly, mode)
    assert cells == [want_cells[k] for k in cols]
    assert proofs == [tau_closed_form(oracle, S.quotient(poly, k)) for k in cols]
    assert (cells, proofs) == ([full[0][0][k] for k in cols], [full[0][1][k] for k in cols])   # the reference of everything below


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_column_sets_in_every_mode(K, gpu_setup, mode, n):
    import torch
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
        for cols in [[0], [127], [63, 64], EVEN, ODD, RANDOM8, ALL]:
            _check(K, torch, gpu_setup, full, mode, n, cols)
            _check(K, torch, gpu_setup, full, mode, n, cols, proofs=False)
            _check(K, torch, gpu_setup, full, mode, n, cols, cells=False)


def test_all_128_columns_are_the_full_call_kernels_included(K, gpu_setup):
    import torch
    mode = S.MODE_REFERENCE
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
        try:
            K.lib().lwkzg_profile_reset()
            K.lib().lwkzg_profile_enable(1)
            K.compute_cells_and_kzg_proofs_batch(_blobs(2, mode), gpu_setup)
            _check(K, torch, gpu_setup, full, mode, 2, ALL)
            K.lib().lwkzg_profile_enable(0)
            kernels = K.capi.profile_report()
            assert not [k for k in NEW_KERNELS if k in kernels] and "k_cells_quotients" in kernels and "k_cells_extend_out" in kernels
            K.lib().lwkzg_profile_reset()
            K.lib().lwkzg_profile_enable(1)
            _check(K, torch, gpu_setup, full, mode, 2, RANDOM8)
            K.lib().lwkzg_profile_enable(0)
            kernels = K.capi.profile_report()
            assert "k_cells_quotients_columns" in kernels and "k_cells_extend_out_columns" in kernels
            assert "k_cells_quotients" not in kernels and "k_cells_extend_out" not in kernels
        finally:
            K.lib().lwkzg_profile_enable(0)
            K.lib().lwkzg_profile_reset()


# ---------------------------------------------------------------------------------------------------------------- slot counts

@pytest.mark.parametrize("mode", [S.MODE_REFERENCE, S.MODE_CKZG])
@pytest.mark.parametrize("n,c", [(1, 1), (1, 8), (2, 4), (1, 9), (3, 3), (5, 3), (1, 127), (3, 43)])
def test_slot_counts_new_to_the_cells_pipeline(K, gpu_setup, mode, n, c):
    """n c = 1, 8 (the cooperative kernel's last), 9 (the accumulation kernels' first), 15, 127, 129"""
    import torch
    cols = sorted(random.Random(100 * n + c).sample(range(128), c))
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
        _check(K, torch, gpu_setup, full, mode, n, cols, cells=False, first=3)
        _check(K, torch, gpu_setup, full, mode, n, cols, first=5)


# ---------------------------------------------------------------------------------------------------------------- chunk boundaries

@pytest.mark.parametrize("c,n,cells", [(100, 11, True), (64, 17, True), (3, 342, False), (1, 513, True), (128, 9, True)])
def test_one_blob_past_every_chunk_of_the_plan(K, gpu_setup, c, n, cells):
    import torch
    assert n == _chunk(c, cells) + 1
    mode = S.MODE_CKZG if c in (100, 3) else S.MODE_REFERENCE
    cols = sorted(random.Random(c).sample(range(128), c))
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
        _check(K, torch, gpu_setup, full, mode, n, cols, cells=cells)


# ---------------------------------------------------------------------------------------------------------------- host forms

def test_the_host_form_across_the_plans_slice(K, gpu_setup):
    import torch
    mode, cols = S.MODE_REFERENCE, RANDOM8
    n = _slice(_chunk(8, True), 131072 + 8 * CELL + 8 * 48 + 4, 10 ** 6) + 1
    assert n == 385
    data = _blobs(n, mode)
    with _mode(K, gpu_setup, mode):
        got = K.compute_cells_and_kzg_proofs_columns(data, cols, gpu_setup)
        dev_c, dev_p, status = _columns(K, torch, data, n, cols, gpu_setup)
        assert status == [0] * n
        assert b"".join(b"".join(cs) for cs, _ in got) == dev_c and b"".join(b"".join(ps) for _, ps in got) == dev_p
        assert (dev_c, dev_p) == _want(_full(K, gpu_setup, mode), n, cols)
        # either output alone, a few blobs
        (cs, ps), = K.compute_cells_and_kzg_proofs_columns(data[:131072], cols, gpu_setup, proofs=False)
        assert ps is None and b"".join(cs) == dev_c[:8 * CELL]
        (cs, ps), = K.compute_cells_and_kzg_proofs_columns(data[:131072], cols, gpu_setup, cells=False)
        assert cs is None and b"".join(ps) == dev_p[:8 * 48]


# ---------------------------------------------------------------------------------------------------------------- bad input

@pytest.mark.parametrize("c,n,bad", [(2, 3, 1), (100, 11, 10)])
def test_an_element_not_below_r_fails_its_blob_alone(K, gpu_setup, c, n, bad):
    """c-kzg mode; the middle blob of three, and the blob behind the chunk boundary of c = 100"""
    import torch
    mode = S.MODE_CKZG
    cols = sorted(random.Random(7 * c).sample(range(128), c))
    blobs = [_blob(b % DISTINCT, mode) for b in range(n)]
    spoilt = bytearray(blobs[bad])
    spoilt[32 * 100:32 * 101] = R.to_bytes(32, "little")
    blobs[bad] = bytes(spoilt)
    data = b"".join(blobs)
    with _mode(K, gpu_setup, mode):
        want_c, want_p = _want(_full(K, gpu_setup, mode), n, cols)
        cells = C.create_string_buffer(b"\x5a" * (n * c * CELL), n * c * CELL)
        proofs = C.create_string_buffer(b"\x5a" * (n * c * 48), n * c * 48)
        first_bad = C.c_size_t(12345)
        rc = K.lib().lwkzg_compute_cells_and_kzg_proofs_columns(cells, proofs, data, n, (C.c_uint64 * c)(*cols), c, gpu_setup.ref(),
                                                                C.byref(first_bad))
        assert rc == K.C_KZG_BADARGS and first_bad.value == bad
        assert cells.raw == b"\x5a" * (n * c * CELL) and proofs.raw == b"\x5a" * (n * c * 48)
        got_c, got_p, status = _columns(K, torch, data, n, cols, gpu_setup)
    assert status == [K.C_KZG_BADARGS if b == bad else 0 for b in range(n)]
    for b in range(n):
        if b != bad:
            assert got_c[b * c * CELL:(b + 1) * c * CELL] == want_c[b * c * CELL:(b + 1) * c * CELL], b
            assert got_p[b * c * 48:(b + 1) * c * 48] == want_p[b * c * 48:(b + 1) * c * 48], b


# ---------------------------------------------------------------------------------------------------------------- recover

def _given(full, n, idx, first=0):
    return b"".join(full[(first + b) % DISTINCT][0][k] for b in range(n) for k in idx)


def _recover(K, torch, idx, given, n, cols, ts, cells=True, proofs=True):
    c = len(cols)
    din = _dev(torch, given)
    dc = torch.full((n * c * CELL,), 0x5a, dtype=torch.uint8, device="cuda") if cells else None
    dp = torch.full((n * c * 48,), 0x5a, dtype=torch.uint8, device="cuda") if proofs else None
    ds = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    K.recover_cells_and_kzg_proofs_columns_device(dc.data_ptr() if cells else None, dp.data_ptr() if proofs else None, idx, din.data_ptr(), n, cols,
                                                  ts, None, ds.data_ptr())
    torch.cuda.synchronize()
    return _host(dc) if cells else None, _host(dp) if proofs else None, ds.cpu().tolist()


GIVEN100 = sorted(random.Random(11).sample(range(128), 100))
MISSING28 = [k for k in range(128) if k not in GIVEN100]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("idx,cols", [(EVEN, ODD), (GIVEN100, MISSING28)], ids=["even-odd", "100-28"])
def test_recover_the_missing_columns(K, gpu_setup, mode, idx, cols):
    """n = 1 and one blob past the chunk (two workspace slots per blob whatever is wanted)"""
    import torch
    past = _chunk(len(cols), True, recover=True) + 1
    assert past == (17 if len(cols) == 64 else 37)
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
        for n in (1, past):
            got_c, got_p, status = _recover(K, torch, idx, _given(full, n, idx, first=2), n, cols, gpu_setup)
            assert status == [0] * n and (got_c, got_p) == _want(full, n, cols, first=2), n
        # the host form, and the outputs on their own
        got = K.recover_cells_and_kzg_proofs_columns(idx, _given(full, 2, idx), 2, cols, gpu_setup)
        assert (b"".join(b"".join(cs) for cs, _ in got), b"".join(b"".join(ps) for _, ps in got)) == _want(full, 2, cols)
        assert _recover(K, torch, idx, _given(full, 2, idx), 2, cols, gpu_setup, proofs=False)[0] == _want(full, 2, cols)[0]


def test_recover_proofs_only_past_a_chunk_that_its_scratch_bounds(K, gpu_setup):
    """c = 1 without cells: a compute call takes 1024 blobs to a pass, the recovery 512, for its two slots of scratch per blob"""
    import torch
    mode, n = S.MODE_REFERENCE, _chunk(1, False, recover=True) + 1
    assert n == 513
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
        got_c, got_p, status = _recover(K, torch, EVEN, _given(full, n, EVEN), n, [77], gpu_setup, cells=False)
        assert status == [0] * n and got_p == _want(full, n, [77])[1]


def _alter(cells, i, t, mode):
    """element t of the i-th given cell replaced by itself + 1"""
    out = bytearray(cells)
    at = CELL * i + 32 * t
    out[at:at + 32] = S.to_bytes((S.element(bytes(out[at:at + 32]), mode) + 1) % R, mode)
    return bytes(out)


@pytest.mark.parametrize("mode", [S.MODE_REFERENCE, S.MODE_CKZG])
def test_recover_inconsistent_cells_fail_whatever_the_columns_and_given_columns_come_back(K, gpu_setup, mode):
    import torch
    idx = sorted(random.Random(12).sample(range(128), 65))
    code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
        good = _given(full, 3, idx)
        per = [good[b * 65 * CELL:(b + 1) * 65 * CELL] for b in range(3)]
        per[1] = _alter(per[1], 30, 7, mode)
        absent = [k for k in range(128) if k not in idx]
        for cols in ([idx[30]], [idx[0]], absent[:3], ALL):
            c = len(cols)
            out_c = C.create_string_buffer(b"\x5a" * (3 * c * CELL), 3 * c * CELL)
            out_p = C.create_string_buffer(b"\x5a" * (3 * c * 48), 3 * c * 48)
            first_bad = C.c_size_t(12345)
            rc = K.lib().lwkzg_recover_cells_and_kzg_proofs_columns(out_c, out_p, (C.c_uint64 * 65)(*idx), b"".join(per), 65, 3,
                                                                    (C.c_uint64 * c)(*cols), c, gpu_setup.ref(), C.byref(first_bad))
            assert rc == code and first_bad.value == 1, cols
            assert out_c.raw == b"\x5a" * (3 * c * CELL) and out_p.raw == b"\x5a" * (3 * c * 48)
            got_c, got_p, status = _recover(K, torch, idx, b"".join(per), 3, cols, gpu_setup)
            assert status == [0, code, 0], cols
            want_c, want_p = _want(full, 3, cols)
            for b in (0, 2):
                assert got_c[b * c * CELL:(b + 1) * c * CELL] == want_c[b * c * CELL:(b + 1) * c * CELL]
                assert got_p[b * c * 48:(b + 1) * c * 48] == want_p[b * c * 48:(b + 1) * c * 48]
        # wanted columns among the given ones: legal, and their cells are the given bytes
        inside = idx[5:25:3]
        got_c, got_p, status = _recover(K, torch, idx, good, 3, inside, gpu_setup)
        assert status == [0] * 3 and (got_c, got_p) == _want(full, 3, inside)
        assert got_c == b"".join(good[(b * 65 + idx.index(k)) * CELL:(b * 65 + idx.index(k) + 1) * CELL] for b in range(3) for k in inside)


# ---------------------------------------------------------------------------------------------------------------- engines

def test_the_bucket_engine(K, gpu_setup, bucket_setup):
    import torch
    for mode in (S.MODE_REFERENCE, S.MODE_CKZG):
        with _mode(K, gpu_setup, mode):
            full = _full(K, gpu_setup, mode)   # the same setup: the same bytes on every engine
        with _mode(K, bucket_setup, mode):
            _check(K, torch, bucket_setup, full, mode, 3, sorted(random.Random(43).sample(range(128), 43)))
            _check(K, torch, bucket_setup, full, mode, 1, [9], cells=False)
            got = K.recover_cells_and_kzg_proofs_columns(EVEN, _given(full, 2, EVEN), 2, ODD, bucket_setup)
            assert (b"".join(b"".join(cs) for cs, _ in got), b"".join(b"".join(ps) for _, ps in got)) == _want(full, 2, ODD)


def test_a_lagrange_only_table_in_ckzg_mode(K, gpu_setup):
    """the quotients become evaluations in front of the MSM, through ws.scalars and ws.fr of the same slots: 129 and 15 of them"""
    import torch
    mode = S.MODE_CKZG
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        ts.set_mode(K.MODE_CKZG)
        ts.enable_direct_table_forms(10, 2)
        assert ts.direct_table_forms() == 2
        _check(K, torch, ts, full, mode, 3, sorted(random.Random(44).sample(range(128), 43)))
        _check(K, torch, ts, full, mode, 5, [1, 64, 126], cells=False)
        _check(K, torch, ts, full, mode, 11, sorted(random.Random(45).sample(range(128), 100)))
        got_c, got_p, status = _recover(K, torch, GIVEN100, _given(full, 2, GIVEN100), 2, MISSING28, ts)
        assert status == [0, 0] and (got_c, got_p) == _want(full, 2, MISSING28)
    finally:
        ts.free()


@pytest.mark.parametrize("path,closed", [(SETUP_TAU2_PATH, lambda o, q: tau_closed_form(o, q, tau=M.TAU2)),
                                         (SETUP_UNSTRUCTURED_PATH, unstructured_closed_form)], ids=["tau2", "unstructured"])
def test_the_second_and_the_unstructured_setup(K, gpu_setup, oracle, path, closed):
    import torch
    mode, cols = S.MODE_REFERENCE, [2, 65, 127]
    ts = K.TrustedSetup.from_file(path)
    try:
        with _mode(K, ts, mode):
            full = _full(K, ts, mode, key=path)
            _check(K, torch, ts, full, mode, 3, cols)
        poly = S.poly_from_blob(_blob(0, mode), mode)
        assert [full[0][1][k] for k in cols] == [closed(oracle, S.quotient(poly, k)) for k in cols]
    finally:
        ts.free()


# ---------------------------------------------------------------------------------------------------------------- FK20

def _fk20_kernels(K, run):
    K.lib().lwkzg_profile_reset()
    K.lib().lwkzg_profile_enable(1)
    try:
        out = run()
    finally:
        K.lib().lwkzg_profile_enable(0)
    kernels = K.capi.profile_report()
    K.lib().lwkzg_profile_reset()
    return out, sorted(k for k in kernels if k.startswith("k_fk20")), kernels


@pytest.mark.parametrize("min_blobs,n,below,above", [(1, 1, 127, 128), (2, 3, 85, 86)])
def test_fk20_serves_a_call_from_as_many_proofs_as_its_threshold_brings(K, gpu_setup, min_blobs, n, below, above):
    import torch
    mode = S.MODE_REFERENCE
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)   # the MSM engine's bytes
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, 0, min_blobs)
        with _mode(K, ts, mode):
            for c, on in [(below, False), (above, True)]:
                cols = sorted(random.Random(c).sample(range(128), c))
                _, fk, kernels = _fk20_kernels(K, lambda: _check(K, torch, ts, full, mode, n, cols))
                if not on:
                    assert fk == [] and "k_cells_quotients_columns" in kernels, c
                elif c == 128:   # all 128: the full call
                    assert fk == ["k_fk20_coeffs", "k_fk20_msm", "k_fk20_transforms"] and not [k for k in NEW_KERNELS if k in kernels]
                else:
                    assert fk == ["k_fk20_coeffs", "k_fk20_columns_compress", "k_fk20_msm", "k_fk20_transforms"], c
                    assert "k_cells_quotients_columns" not in kernels and "k_finalize_compress" not in kernels
            # the recovery follows the same rule
            cols = sorted(random.Random(1).sample(range(128), above))
            (got_c, got_p, status), fk, _ = _fk20_kernels(K, lambda: _recover(K, torch, EVEN, _given(full, n, EVEN), n, cols, ts))
            assert status == [0] * n and (got_c, got_p) == _want(full, n, cols) and "k_fk20_msm" in fk
            # a full call's report names none of the new kernels
            _, fk, kernels = _fk20_kernels(K, lambda: K.compute_cells_and_kzg_proofs_batch(_blobs(n + 1, mode), ts))
            assert fk == ["k_fk20_coeffs", "k_fk20_msm", "k_fk20_transforms"] and not [k for k in NEW_KERNELS if k in kernels]
    finally:
        ts.set_cell_proof_engine(K.CELL_PROOFS_MSM)
        ts.free()


# ---------------------------------------------------------------------------------------------------------------- streams

def test_the_callers_stream_and_two_lists_back_to_back(K, gpu_setup):
    """the list travels by value: the second call's list does not reach the first call's kernels, with nothing between the two calls"""
    import torch
    mode, n = S.MODE_CKZG, 20
    first, second = [1, 2, 3, 64, 65, 90, 101, 127], [0, 5, 63, 64, 100, 110, 120, 126]
    with _mode(K, gpu_setup, mode):
        full = _full(K, gpu_setup, mode)
        db = _dev(torch, _blobs(n, mode))
        out = [(torch.full((n * 8 * CELL,), 0x5a, dtype=torch.uint8, device="cuda"), torch.full((n * 8 * 48,), 0x5a, dtype=torch.uint8, device="cuda"),
                torch.full((n,), -7, dtype=torch.int32, device="cuda")) for _ in range(2)]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for (dc, dp, ds), cols in zip(out, (first, second)):
                K.compute_cells_and_kzg_proofs_columns_device(dc.data_ptr(), dp.data_ptr(), db.data_ptr(), n, cols, gpu_setup, s.cuda_stream,
                                                              ds.data_ptr())
        s.synchronize()
        for (dc, dp, ds), cols in zip(out, (first, second)):
            assert ds.cpu().tolist() == [0] * n and (_host(dc), _host(dp)) == _want(full, n, cols), cols
