"""GPU: the opt-in FK20 cell proof engine (lwkzg_set_cell_proof_engine). Every call here passes min_blobs = 1 so
that FK20 really runs. The engine's control; its 8192 bases, E and h of a blob against closed forms on the tau = 1337 setup
(lwkzg_fk20_points); proofs against [q_k(tau)]G on three setups; edge blobs, among them the one whose forward transform doubles in one
butterfly and cancels in another; byte equality with the MSM engine across the chunk, on both MSM engines, a Lagrange-only table and the
host slices; status words; the threshold; recovery; two caller streams; and the switch back."""
import contextlib
import ctypes as C
import json
import random

import pytest

import blobs as B
import cells_spec as S
import fk20_spec as F
import make_setups as M
from conftest import P, R, SETUP_PATH, SETUP_TAU2_PATH, SETUP_UNSTRUCTURED_PATH, TAU, tau_closed_form, unstructured_closed_form

pytestmark = pytest.mark.gpu

INF = bytes([0xc0]) + bytes(47)
MODES = [S.MODE_REFERENCE, S.MODE_CKZG]
K_BLOB = 4096 * 32
GIB = 1 << 30


@contextlib.contextmanager
def _mode(K, ts, mode):
    K.lib().lwkzg_settings_set_mode(ts.ref(), mode)
    try:
        yield
    finally:
        K.lib().lwkzg_settings_set_mode(ts.ref(), -1)


@contextlib.contextmanager
def _fk20(K, ts, window_bits=0, min_blobs=1):
    ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, window_bits, min_blobs)
    try:
        yield
    finally:
        ts.set_cell_proof_engine(K.CELL_PROOFS_MSM)


@pytest.fixture(scope="module")
def fk(K):
    """a settings object of its own on the tau = 1337 setup with the FK20 engine on at the default width"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, 0, 1)
    yield ts
    ts.free()


def _blob(seed, mode):
    return B.synthetic_blob(seed, big_endian=mode == S.MODE_REFERENCE)


def _want_cells(blob, mode):
    return S.cells_bytes(S.poly_from_blob(blob, mode), mode)


def _want_proofs(oracle, blob, mode, closed=lambda o, q: tau_closed_form(o, q)):
    p = S.poly_from_blob(blob, mode)
    return [closed(oracle, S.quotient(p, k)) for k in range(128)]


def _compress(rec):
    """a 97-byte record flag | x | y of lwkzg_fk20_points -> the 48 compressed bytes"""
    assert len(rec) == 97 and rec[0] in (0, 1)
    if rec[0]:
        assert rec[1:] == bytes(96)
        return INF
    x, y = rec[1:49], int.from_bytes(rec[49:], "big")
    return bytes([x[0] | 0x80 | (0x20 if P - y < y else 0)]) + x[1:]


def _dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _device_proofs(K, torch, data, n, ts, stream=None):
    """the proofs of n device-resident blobs (no cells) and the status words"""
    db = _dev(torch, data)
    dp = torch.zeros(n * 128 * 48, dtype=torch.uint8, device="cuda")
    ds = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    K.compute_cells_and_kzg_proofs_batch_device(None, dp.data_ptr(), db.data_ptr(), n, ts, stream, ds.data_ptr())
    torch.cuda.synchronize()
    return bytes(dp.cpu().numpy()), ds.cpu().tolist()


def _cyclic(n, mode, first=900):
    """n blobs drawn cyclically from 17 distinct ones, so that a misplaced blob shows"""
    distinct = [_blob(first + i, mode) for i in range(17)]
    return b"".join(distinct[i % 17] for i in range(n))


# ---------------------------------------------------------------------------------------------------------------- engine control

def test_engine_control(K):
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        assert ts.cell_proof_engine() == K.CELL_PROOFS_MSM and ts.fk20_table_bytes() == 0
        ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, 0, 1)
        assert ts.cell_proof_engine() == K.CELL_PROOFS_FK20
        size = ts.fk20_table_bytes()
        assert size == 8192 * 32 * 128 * 112 and 0 < size < 8 * GIB   # the default width: 32 windows of 128 rows
        ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, 0, 1)           # twice: harmless
        assert ts.cell_proof_engine() == K.CELL_PROOFS_FK20 and ts.fk20_table_bytes() == size
        with pytest.raises(K.KzgError) as e:
            ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, 99, 1)
        assert e.value.rc == K.C_KZG_BADARGS and ts.cell_proof_engine() == K.CELL_PROOFS_FK20
        ts.set_cell_proof_engine(K.CELL_PROOFS_MSM)
        assert ts.cell_proof_engine() == K.CELL_PROOFS_MSM and ts.fk20_table_bytes() == 0
        ts.set_cell_proof_engine(K.CELL_PROOFS_MSM)                   # and off twice
        with pytest.raises(K.KzgError):
            ts.fk20_points(0)
    finally:
        ts.free()


# ---------------------------------------------------------------------------------------------------------------- bases and stages

def test_bases_against_the_closed_form(K, fk, oracle):
    got = fk.fk20_points(0)
    rnd = random.Random(8192)
    sample = [(0, 0), (63, 127), (0, 64), (63, 1)]
    while len(sample) < 48:
        im = (rnd.randrange(64), rnd.randrange(128))
        if im not in sample:
            sample.append(im)
    for i, m in sample:
        k = sum(pow(F.W, m * j, R) * pow(TAU, 64 * (62 - j) + i, R) for j in range(63)) % R
        assert _compress(got[128 * i + m]) == oracle.g1_generator_mul(k), (i, m)


@pytest.mark.parametrize("mode", MODES)
def test_stages_against_the_closed_forms(K, fk, oracle, mode):
    blob = _blob(1000, mode)
    p = S.poly_from_blob(blob, mode)
    G = [pow(TAU, t, R) for t in range(4096)]   # the setup's points as multiples of the generator
    with _mode(K, fk, mode):
        h = fk.fk20_points(2, blob)
        e = fk.fk20_points(1, blob)
    want_h = F.h_direct(p, G)
    assert want_h[63] == 0 and _compress(h[63]) == INF
    assert [_compress(x) for x in h] == [oracle.g1_generator_mul(k) for k in want_h]
    want_e = F.e_points(p, F.bases(G))
    assert [_compress(x) for x in e] == [oracle.g1_generator_mul(k) for k in want_e]


# ---------------------------------------------------------------------------------------------------------------- proofs

@pytest.mark.parametrize("mode", MODES)
def test_proofs_match_the_closed_form_on_the_default_setup(K, fk, gpu_setup, oracle, mode):
    blobs = [_blob(1010 + i, mode) for i in range(2)]
    with _mode(K, fk, mode), _mode(K, gpu_setup, mode):
        got = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), fk)
        msm = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), gpu_setup)
    for b, (cells, proofs) in zip(blobs, got):
        assert proofs == _want_proofs(oracle, b, mode)
    assert got[0][0] == _want_cells(blobs[0], mode)
    assert got == msm   # the cells are unchanged, and so are the bytes of the proofs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["tau2", "unstructured"])
def test_proofs_on_the_second_and_the_unstructured_setup(K, gpu_setup, oracle, mode, which):
    path, closed, bits = {"tau2": (SETUP_TAU2_PATH, lambda o, q: tau_closed_form(o, q, tau=M.TAU2), 6),
                          "unstructured": (SETUP_UNSTRUCTURED_PATH, unstructured_closed_form, 4)}[which]
    blobs = [_blob(1020 + i, mode) for i in range(2)]
    ts = K.TrustedSetup.from_file(path)
    try:
        ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, bits, 1)
        with _mode(K, ts, mode), _mode(K, gpu_setup, mode):
            got = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), ts)
            cells = [c for c, _ in K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), gpu_setup, proofs=False)]
        for b, (_, proofs) in zip(blobs, got):
            assert proofs == _want_proofs(oracle, b, mode, closed), path
        assert [c for c, _ in got] == cells   # (cells do not depend on the setup)
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
        "doubles_and_cancels": (S.blob_from_poly(F.edge_polynomial(TAU), mode), "edge"),
    }
    if mode == S.MODE_REFERENCE:
        vals = [rnd.randrange(R, 2 ** 256) if i % 3 == 0 else rnd.randrange(R) for i in range(4096)]
        out["elements_at_least_r"] = (b"".join(v.to_bytes(32, "big") for v in vals), None)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_edge_blobs(K, fk, oracle, mode):
    gen, two = oracle.g1_generator_mul(1), oracle.g1_generator_mul(2)
    for name, (blob, kind) in _edge_blobs(mode).items():
        with _mode(K, fk, mode):
            cells, proofs = K.compute_cells_and_kzg_proofs(blob, fk)
        assert cells == _want_cells(blob, mode), name
        if kind == "inf":
            assert proofs == [INF] * 128, name
        elif kind == "gen":
            assert proofs == [gen] * 128, name
        elif kind == "edge":   # proof_k = [1 + (w^32)^rev7(k)]G: h_0 = h_32 = G, every other h_u at infinity
            want = [oracle.g1_generator_mul((1 + pow(F.W, 32 * S.rev(k, 7), R)) % R) for k in range(128)]
            assert proofs == want and proofs.count(two) == 32 and proofs.count(INF) == 32, name
            with _mode(K, fk, mode):
                h = [_compress(x) for x in fk.fk20_points(2, blob)]
            assert h == [gen if u in (0, 32) else INF for u in range(64)]
        else:
            assert proofs == _want_proofs(oracle, blob, mode), name
    if mode == S.MODE_REFERENCE:   # elements >= r are reduced: the same outputs as the reduced blob
        blob = _edge_blobs(mode)["elements_at_least_r"][0]
        reduced = b"".join((int.from_bytes(blob[32 * i:32 * i + 32], "big") % R).to_bytes(32, "big") for i in range(4096))
        with _mode(K, fk, mode):
            assert K.compute_cells_and_kzg_proofs(blob, fk) == K.compute_cells_and_kzg_proofs(reduced, fk)


# ---------------------------------------------------------------------------------------------------------------- equality with the MSM engine

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 9, "chunk+1"])
def test_device_calls_equal_the_msm_engine(K, fk, gpu_setup, mode, n):
    import torch
    n = K.fk20_chunk_blobs() + 1 if n == "chunk+1" else n
    data = _cyclic(n, mode)
    with _mode(K, fk, mode), _mode(K, gpu_setup, mode):
        got, st = _device_proofs(K, torch, data, n, fk)
        want, st_msm = _device_proofs(K, torch, data, n, gpu_setup)
    assert st == [0] * n == st_msm
    assert [i for i in range(n) if got[6144 * i:6144 * (i + 1)] != want[6144 * i:6144 * (i + 1)]] == []


@pytest.mark.parametrize("mode", MODES)
def test_on_the_bucket_engine(K, bucket_setup, mode):
    blobs = _cyclic(3, mode, first=1100)
    with _mode(K, bucket_setup, mode):
        want = K.compute_cells_and_kzg_proofs_batch(blobs, bucket_setup)
        with _fk20(K, bucket_setup, 7):   # (the bases are committed by the bucket engine)
            got = K.compute_cells_and_kzg_proofs_batch(blobs, bucket_setup)
    assert got == want


def test_on_a_lagrange_only_table(K):
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        ts.set_mode(K.MODE_CKZG)
        ts.enable_direct_table_forms(10, 2)
        assert ts.direct_table_forms() == 2
        blobs = _cyclic(3, S.MODE_CKZG, first=1120)
        want = K.compute_cells_and_kzg_proofs_batch(blobs, ts)
        with _fk20(K, ts, 6):
            assert K.compute_cells_and_kzg_proofs_batch(blobs, ts) == want
    finally:
        ts.free()


def test_host_batch_across_its_slice(K, fk, gpu_setup):
    n = 65   # the host-pointer forms upload 64 blobs at a time
    blobs = _cyclic(n, S.MODE_REFERENCE, first=1140)
    with _mode(K, fk, S.MODE_REFERENCE), _mode(K, gpu_setup, S.MODE_REFERENCE):
        got = K.compute_cells_and_kzg_proofs_batch(blobs, fk)
        want = K.compute_cells_and_kzg_proofs_batch(blobs, gpu_setup)
    assert [i for i in range(n) if got[i] != want[i]] == []


# ---------------------------------------------------------------------------------------------------------------- status words

def test_noncanonical_element_in_the_middle_of_a_batch_and_behind_a_chunk_boundary(K, fk, gpu_setup):
    import torch
    mode = S.MODE_CKZG
    blobs = [_blob(1200 + i, mode) for i in range(5)]
    bad = bytearray(blobs[2])
    bad[32 * 100:32 * 101] = R.to_bytes(32, "little")
    blobs[2] = bytes(bad)
    data = b"".join(blobs)
    with _mode(K, fk, mode), _mode(K, gpu_setup, mode):
        cells = C.create_string_buffer(5 * 128 * 2048)
        proofs = C.create_string_buffer(5 * 128 * 48)
        first_bad = C.c_size_t(12345)
        rc = K.lib().lwkzg_compute_cells_and_kzg_proofs_batch(cells, proofs, data, 5, fk.ref(), C.byref(first_bad))
        assert rc == K.C_KZG_BADARGS and first_bad.value == 2
        assert cells.raw == bytes(len(cells.raw)) and proofs.raw == bytes(len(proofs.raw))   # nothing written
        got, st = _device_proofs(K, torch, data, 5, fk)
        want, st_msm = _device_proofs(K, torch, data, 5, gpu_setup)
        assert st == st_msm and [s != 0 for s in st] == [False, False, True, False, False]
        assert [got[6144 * i:6144 * (i + 1)] == want[6144 * i:6144 * (i + 1)] for i in (0, 1, 3, 4)] == [True] * 4
        # the first blob behind a chunk boundary
        chunk = K.fk20_chunk_blobs()
        n = chunk + 2
        many = bytearray(_cyclic(n, mode, first=1210))
        many[chunk * K_BLOB + 32 * 7:chunk * K_BLOB + 32 * 8] = R.to_bytes(32, "little")
        got, st = _device_proofs(K, torch, bytes(many), n, fk)
        assert [i for i, s in enumerate(st) if s != 0] == [chunk] and st[chunk] == K.C_KZG_BADARGS
        near = bytes(many[(chunk - 1) * K_BLOB:(chunk + 2) * K_BLOB])
        want, st_msm = _device_proofs(K, torch, near, 3, gpu_setup)
        assert st_msm == st[chunk - 1:]
        for i in (0, 2):
            assert got[6144 * (chunk - 1 + i):6144 * (chunk + i)] == want[6144 * i:6144 * (i + 1)], i


# ---------------------------------------------------------------------------------------------------------------- threshold

def test_threshold(K, fk, gpu_setup):
    import torch
    mode = S.MODE_REFERENCE
    fk.set_cell_proof_engine(K.CELL_PROOFS_FK20, 0, 4)
    try:
        with _mode(K, fk, mode), _mode(K, gpu_setup, mode):
            seen = {}
            for n in (3, 4):
                data = _cyclic(n, mode, first=1300)
                want, _ = _device_proofs(K, torch, data, n, gpu_setup)
                K.lib().lwkzg_profile_reset()
                K.lib().lwkzg_profile_enable(1)
                got, st = _device_proofs(K, torch, data, n, fk)
                K.lib().lwkzg_profile_enable(0)
                seen[n] = sorted(k for k in K.capi.profile_report() if k.startswith("k_fk20"))
                assert got == want and st == [0] * n, n
        assert seen[3] == []
        assert seen[4] == ["k_fk20_coeffs", "k_fk20_msm", "k_fk20_transforms"]
    finally:
        K.lib().lwkzg_profile_enable(0)
        K.lib().lwkzg_profile_reset()
        fk.set_cell_proof_engine(K.CELL_PROOFS_FK20, 0, 1)


# ---------------------------------------------------------------------------------------------------------------- recovery

@pytest.mark.parametrize("given", [64, 100])
def test_recovery_equals_compute(K, fk, given):
    mode = S.MODE_CKZG
    blobs = [_blob(1400 + i, mode) for i in range(2)]
    idx = sorted(random.Random(given).sample(range(128), given))
    with _mode(K, fk, mode):
        want = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), fk)
        have = b"".join(b"".join(cells[k] for k in idx) for cells, _ in want)
        assert K.recover_cells_and_kzg_proofs_batch(idx, have, 2, fk) == want


# ---------------------------------------------------------------------------------------------------------------- two caller streams

def test_two_calls_on_two_caller_streams(K, fk):
    import torch
    mode = S.MODE_REFERENCE
    da, db = _cyclic(3, mode, first=1500), _cyclic(2, mode, first=1510)
    with _mode(K, fk, mode):
        wa, _ = _device_proofs(K, torch, da, 3, fk)
        wb, _ = _device_proofs(K, torch, db, 2, fk)
        bufs = []
        for data, n in ((da, 3), (db, 2)):
            bufs.append((_dev(torch, data), torch.zeros(n * 6144, dtype=torch.uint8, device="cuda"),
                         torch.full((n,), -7, dtype=torch.int32, device="cuda"), n))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for (din, dp, ds, n), s in zip(bufs, (s1, s2)):   # no host synchronisation between the two calls
            K.compute_cells_and_kzg_proofs_batch_device(None, dp.data_ptr(), din.data_ptr(), n, fk, s.cuda_stream, ds.data_ptr())
        s1.synchronize()
        s2.synchronize()
    assert bytes(bufs[0][1].cpu().numpy()) == wa and bufs[0][2].cpu().tolist() == [0] * 3
    assert bytes(bufs[1][1].cpu().numpy()) == wb and bufs[1][2].cpu().tolist() == [0] * 2


# ---------------------------------------------------------------------------------------------------------------- and back

def test_after_the_switch_back_the_outputs_are_the_msm_engines(K, gpu_setup, oracle):
    mode = S.MODE_REFERENCE
    blob = _blob(1600, mode)
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        with _mode(K, ts, mode), _mode(K, gpu_setup, mode):
            before = K.compute_cells_and_kzg_proofs(blob, ts)
            with _fk20(K, ts, 4):
                during = K.compute_cells_and_kzg_proofs(blob, ts)
            K.lib().lwkzg_profile_reset()
            K.lib().lwkzg_profile_enable(1)
            after = K.compute_cells_and_kzg_proofs(blob, ts)
            K.lib().lwkzg_profile_enable(0)
            kernels = K.capi.profile_report()
            assert before == during == after == K.compute_cells_and_kzg_proofs(blob, gpu_setup)
        assert after[1] == _want_proofs(oracle, blob, mode)
        assert not [k for k in kernels if k.startswith("k_fk20")] and "k_cells_quotients" in kernels
        assert ts.cell_proof_engine() == K.CELL_PROOFS_MSM and ts.fk20_table_bytes() == 0
    finally:
        K.lib().lwkzg_profile_enable(0)
        K.lib().lwkzg_profile_reset()
        ts.free()
