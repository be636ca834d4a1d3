"""GPU: the mixed recovery (lwkzg_recover_cells_and_kzg_proofs_mixed, _mixed_device: n blobs, every one through an index set of its
own) in both modes. Every expected output is lwkzg_compute_cells_and_kzg_proofs_batch's for the original blobs, computed once per mode
for a pool of 17 blobs (tests/test_gpu_cells.py pins that call to the Python restatement); the shared-set recovery is the second
yardstick. Byte for byte, no tolerance: ragged inputs, repeated sets, sets and offsets that change across the 8-blob proof chunk and
the 64-blob host slice, outputs left out, bad inputs in the middle, two calls back to back on one stream, shared-set calls around a mixed one on one stream, both MSM engines, FK20 and the round trip through the cell proof verifier."""
import contextlib
import ctypes as C
import random

import pytest

import blobs as B
import cells_spec as S
from conftest import R, SETUP_PATH

pytestmark = pytest.mark.gpu

MODES = [S.MODE_REFERENCE, S.MODE_CKZG]
CELL = 2048
POOL = 17


@contextlib.contextmanager
def _mode(K, ts, mode):
    K.lib().lwkzg_settings_set_mode(ts.ref(), mode)
    try:
        yield
    finally:
        K.lib().lwkzg_settings_set_mode(ts.ref(), -1)


_pools = {}


def _pool(K, ts, mode):
    """[(cells, proofs)] of the pool's blobs in `mode`, computed once and never changed"""
    if mode not in _pools:
        with _mode(K, ts, mode):
            blobs = b"".join(B.synthetic_blob(7000 + i, big_endian=mode == S.MODE_REFERENCE) for i in range(POOL))
            _pools[mode] = tuple((tuple(c), tuple(p)) for c, p in K.compute_cells_and_kzg_proofs_batch(blobs, ts))
    return _pools[mode]


def _want(pool, n, first=0):
    """what a call on blobs first, first + 1, ... of the pool (cyclically) gives"""
    return [(list(pool[(first + b) % POOL][0]), list(pool[(first + b) % POOL][1])) for b in range(n)]


def _pick(count, seed):
    return sorted(random.Random(seed).sample(range(128), count))


def _given(want, lists):
    """per blob, the cells its list names, concatenated"""
    return [b"".join(w[0][k] for k in lst) for w, lst in zip(want, lists)]


def _bad_code(K, mode):
    return K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR


def _alter(cells, i, t, mode, value=None):
    """element t of the i-th given cell replaced (by value, or by itself + 1)"""
    out = bytearray(cells)
    at = CELL * i + 32 * t
    v = (S.element(bytes(out[at:at + 32]), mode) + 1) % R if value is None else value
    out[at:at + 32] = S.to_bytes(v, mode)
    return bytes(out)


def _dev(torch, data):
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


class _DeviceCall:
    """the buffers of one device call, made before it and read after it"""

    def __init__(self, torch, lists, per, cells_out=True, proofs=True):
        self.n, self.lists = len(lists), lists
        n = max(self.n, 1)
        self.din = _dev(torch, b"".join(per))
        self.dc = torch.zeros(n * 128 * CELL, dtype=torch.uint8, device="cuda") if cells_out else None
        self.dp = torch.zeros(n * 128 * 48, dtype=torch.uint8, device="cuda") if proofs else None
        self.ds = torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def enqueue(self, K, ts, stream=None):
        K.recover_cells_and_kzg_proofs_mixed_device(self.dc.data_ptr() if self.dc is not None else None,
                                                    self.dp.data_ptr() if self.dp is not None else None, self.lists, self.din.data_ptr(), ts,
                                                    stream, self.ds.data_ptr())

    def result(self, K):
        cr = bytes(self.dc.cpu().numpy()) if self.dc is not None else None
        pr = bytes(self.dp.cpu().numpy()) if self.dp is not None else None
        return K.capi._cells_split(cr, pr, self.n), self.ds.cpu().tolist()[:self.n]


class _SharedSetCall(_DeviceCall):
    """the same for the shared-set device call: every blob through lists[0]"""

    def enqueue(self, K, ts, stream=None):
        K.recover_cells_and_kzg_proofs_batch_device(self.dc.data_ptr() if self.dc is not None else None,
                                                    self.dp.data_ptr() if self.dp is not None else None, self.lists[0], self.din.data_ptr(),
                                                    self.n, ts, stream, self.ds.data_ptr())


def _device(K, torch, lists, per, ts, cells_out=True, proofs=True):
    call = _DeviceCall(torch, lists, per, cells_out, proofs)
    torch.cuda.synchronize()
    call.enqueue(K, ts)
    torch.cuda.synchronize()
    return call.result(K)


def _both_forms(K, torch, ts, lists, want):
    per = _given(want, lists)
    assert K.recover_cells_and_kzg_proofs_mixed(lists, per, ts) == want
    got, status = _device(K, torch, lists, per, ts)
    assert status == [0] * len(lists)
    assert got == want


# 1
@pytest.mark.parametrize("mode", MODES)
def test_ragged_input_with_complementary_sets(K, gpu_setup, mode):
    import torch
    pool = _pool(K, gpu_setup, mode)
    with _mode(K, gpu_setup, mode):
        want = _want(pool, 2)
        _both_forms(K, torch, gpu_setup, [list(range(64)), list(range(128))], want)
        _both_forms(K, torch, gpu_setup, [list(range(128)), list(range(64))], want)
        _both_forms(K, torch, gpu_setup, [list(range(64)), list(range(64, 128))], want)


# 2 (and 11: the round trip)
@pytest.mark.parametrize("mode", MODES)
def test_three_blobs_with_a_repeated_set(K, gpu_setup, mode):
    import torch
    pool = _pool(K, gpu_setup, mode)
    a, b = _pick(64, 201), _pick(100, 202)
    lists = [a, b, a]
    with _mode(K, gpu_setup, mode):
        want = _want(pool, 3, first=2)
        per = _given(want, lists)
        assert [K.recover_cells_and_kzg_proofs(lst, ce, gpu_setup) for lst, ce in zip(lists, per)] == want
        _both_forms(K, torch, gpu_setup, lists, want)


def test_recovered_cells_and_proofs_pass_the_verifier(K, gpu_setup):
    mode = S.MODE_CKZG
    lists = [_pick(64, 201), _pick(100, 202), _pick(64, 201)]
    with _mode(K, gpu_setup, mode):
        blobs = [B.synthetic_blob(7100 + i, big_endian=False) for i in range(3)]
        comms = K.blob_to_kzg_commitment_batch(b"".join(blobs), gpu_setup)
        full = K.compute_cells_and_kzg_proofs_batch(b"".join(blobs), gpu_setup, proofs=False)
        got = K.recover_cells_and_kzg_proofs_mixed(lists, _given(full, lists), gpu_setup)
        assert [g[0] for g in got] == [f[0] for f in full]
        cols = list(zip(*[(comms[b], k, got[b][0][k], got[b][1][k]) for b in range(3) for k in range(128)]))
        assert K.verify_cell_kzg_proof_batch(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), gpu_setup) is True
        swapped = list(cols[3])
        swapped[5], swapped[6] = swapped[6], swapped[5]
        assert K.verify_cell_kzg_proof_batch(list(cols[0]), list(cols[1]), list(cols[2]), swapped, gpu_setup) is False


# 3
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [9, 17])
def test_distinct_sets_across_the_proof_chunk(K, gpu_setup, mode, n):
    """blob 8, the first of the second chunk, has 65 cells where the others have 64: the set and the input offset change there"""
    import torch
    pool = _pool(K, gpu_setup, mode)
    lists = [_pick(65 if b == 8 else 64, 300 + b) for b in range(n)]
    assert len(set(map(tuple, lists))) == n
    with _mode(K, gpu_setup, mode):
        _both_forms(K, torch, gpu_setup, lists, _want(pool, n))


# 4
@pytest.mark.parametrize("mode", MODES)
def test_all_sets_equal_is_the_shared_set_call(K, gpu_setup, mode):
    import torch
    pool = _pool(K, gpu_setup, mode)
    idx = _pick(70, 400)
    with _mode(K, gpu_setup, mode):
        want = _want(pool, 3, first=5)
        per = _given(want, [idx] * 3)
        assert K.recover_cells_and_kzg_proofs_batch(idx, b"".join(per), 3, gpu_setup) == want
        _both_forms(K, torch, gpu_setup, [idx] * 3, want)


# 5
@pytest.mark.parametrize("mode", MODES)
def test_cells_only_across_the_host_slice(K, gpu_setup, mode):
    import torch
    pool = _pool(K, gpu_setup, mode)
    n = 65
    sets = [_pick(c, 500 + c) for c in (64, 65, 100, 127, 128)]
    lists = [sets[(b * 3 + b // 5) % 5] for b in range(n)]
    assert lists[63] != lists[64] and len(lists[63]) != len(lists[64])
    with _mode(K, gpu_setup, mode):
        want = [(c, None) for c, _ in _want(pool, n)]
        per = _given(want, lists)
        assert K.recover_cells_and_kzg_proofs_mixed(lists, per, gpu_setup, proofs=False) == want
        got, status = _device(K, torch, lists, per, gpu_setup, proofs=False)
        assert status == [0] * n and got == want


def test_cells_only_across_the_kernels_group_of_256_blobs(K, gpu_setup):
    """a chunk without proofs holds up to 512 blobs and reaches the kernels 256 at a time: blob 256, the first of the second group, has
    a set and a count of its own. Device form: the host form would cut the call into slices of 64"""
    import torch
    mode = S.MODE_CKZG
    pool = _pool(K, gpu_setup, mode)
    n = 257
    sets = [_pick(c, 540 + c) for c in (64, 65, 128)]
    lists = [_pick(99, 539) if b == 256 else sets[b % 3] for b in range(n)]
    with _mode(K, gpu_setup, mode):
        want = [(c, None) for c, _ in _want(pool, n)]
        got, status = _device(K, torch, lists, _given(want, lists), gpu_setup, proofs=False)
        assert status == [0] * n
        assert got == want


@pytest.mark.parametrize("mode", MODES)
def test_proofs_only(K, gpu_setup, mode):
    import torch
    pool = _pool(K, gpu_setup, mode)
    lists = [_pick(64, 520), _pick(90, 521)]
    with _mode(K, gpu_setup, mode):
        want = [(None, p) for _, p in _want(pool, 2, first=9)]
        per = _given(_want(pool, 2, first=9), lists)
        assert K.recover_cells_and_kzg_proofs_mixed(lists, per, gpu_setup, cells_out=False) == want
        got, status = _device(K, torch, lists, per, gpu_setup, cells_out=False)
        assert status == [0, 0] and got == want


# 6
def _rejected_in_the_middle(K, torch, ts, mode, lists, want, per, bad_blob=2):
    """`per`: 5 blobs' given cells with blob 2 spoilt. The host call fails with the mode's code and writes nothing, the device form
    flags blob 2 alone and the other four are right."""
    n = 5
    flat = [k for lst in lists for k in lst]
    out_c = C.create_string_buffer(b"\x5a" * (n * 128 * CELL), n * 128 * CELL)
    out_p = C.create_string_buffer(b"\x5a" * (n * 128 * 48), n * 128 * 48)
    first_bad = C.c_size_t(12345)
    rc = K.lib().lwkzg_recover_cells_and_kzg_proofs_mixed(out_c, out_p, (C.c_uint64 * len(flat))(*flat), b"".join(per),
                                                          (C.c_size_t * n)(*[len(lst) for lst in lists]), n, ts.ref(), C.byref(first_bad))
    assert rc == _bad_code(K, mode) and first_bad.value == bad_blob
    assert out_c.raw == b"\x5a" * (n * 128 * CELL) and out_p.raw == b"\x5a" * (n * 128 * 48)   # nothing written
    got, status = _device(K, torch, lists, per, ts)
    assert [s != 0 for s in status] == [i == bad_blob for i in range(n)]
    assert status[bad_blob] == _bad_code(K, mode)
    assert [g for i, g in enumerate(got) if i != bad_blob] == [w for i, w in enumerate(want) if i != bad_blob]


@pytest.mark.parametrize("mode", MODES)
def test_bad_inputs_in_the_middle_of_five_blobs_with_five_sets(K, gpu_setup, mode):
    """blob 2's set has 65 cells, its neighbours' 64: an altered element makes it inconsistent, which is impossible for them"""
    import torch
    pool = _pool(K, gpu_setup, mode)
    lists = [_pick(65 if b == 2 else 64, 600 + b) for b in range(5)]
    with _mode(K, gpu_setup, mode):
        want = _want(pool, 5, first=11)
        per = _given(want, lists)
        for value in (R, 2 ** 256 - 1):   # never reduced, not in reference mode either
            spoilt = list(per)
            spoilt[2] = _alter(per[2], 31, 63, mode, value=value)
            _rejected_in_the_middle(K, torch, gpu_setup, mode, lists, want, spoilt)
        spoilt = list(per)
        spoilt[2] = _alter(per[2], 40, 7, mode)
        _rejected_in_the_middle(K, torch, gpu_setup, mode, lists, want, spoilt)
        # as the single call answers for that blob
        with pytest.raises(K.KzgError) as e:
            K.recover_cells_and_kzg_proofs(lists[2], spoilt[2], gpu_setup)
        assert e.value.rc == _bad_code(K, mode)


# 7
@pytest.mark.parametrize("mode", MODES)
def test_two_device_calls_back_to_back_on_one_stream(K, gpu_setup, mode):
    """the metadata lifetime: the first call's kernels still see their own sets after the second call has handed over its own"""
    import torch
    pool = _pool(K, gpu_setup, mode)
    lists1, lists2 = [_pick(64, 700), _pick(80, 701)], [_pick(128, 702), _pick(64, 703), _pick(65, 704)]
    want1, want2 = _want(pool, 2, first=3), _want(pool, 3, first=12)
    with _mode(K, gpu_setup, mode):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            call1 = _DeviceCall(torch, lists1, _given(want1, lists1))
            call2 = _DeviceCall(torch, lists2, _given(want2, lists2))
        torch.cuda.synchronize()
        call1.enqueue(K, gpu_setup, s.cuda_stream)   # no synchronisation between the two
        call2.enqueue(K, gpu_setup, s.cuda_stream)
        s.synchronize()
        assert call1.result(K) == (want1, [0, 0])
        assert call2.result(K) == (want2, [0, 0, 0])


def test_shared_set_calls_around_a_mixed_call_on_one_stream(K, gpu_setup):
    """the two kinds of call share one host pipeline, the workspace and the context's tables: a shared-set call with A, a mixed call
    with B and A and a shared-set call with B, on one stream without synchronisation between them. Each call's setup runs behind the
    kernels of the call before it, so all three are right."""
    import torch
    mode = S.MODE_REFERENCE
    pool = _pool(K, gpu_setup, mode)
    a, b = _pick(64, 710), _pick(90, 711)
    wants = [[(c, None) for c, _ in _want(pool, 2, first=f)] for f in (4, 8, 13)]
    with _mode(K, gpu_setup, mode):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            calls = [_SharedSetCall(torch, [a, a], _given(wants[0], [a, a]), proofs=False),
                     _DeviceCall(torch, [b, a], _given(wants[1], [b, a]), proofs=False),
                     _SharedSetCall(torch, [b, b], _given(wants[2], [b, b]), proofs=False)]
        torch.cuda.synchronize()
        for call in calls:   # no synchronisation between them
            call.enqueue(K, gpu_setup, s.cuda_stream)
        s.synchronize()
        for call, want in zip(calls, wants):
            assert call.result(K) == (want, [0, 0])


# 8
def test_empty_call_and_a_repeated_call(K, gpu_setup):
    import torch
    assert K.recover_cells_and_kzg_proofs_mixed([], [], gpu_setup) == []
    l = K.lib()
    assert l.lwkzg_recover_cells_and_kzg_proofs_mixed(None, None, None, None, None, 0, gpu_setup.ref(), None) == K.C_KZG_OK
    assert l.lwkzg_recover_cells_and_kzg_proofs_mixed_device(None, None, None, None, None, 0, gpu_setup.ref(), None, None) == K.C_KZG_OK
    mode = S.MODE_REFERENCE
    pool = _pool(K, gpu_setup, mode)
    lists = [_pick(64, 800), _pick(66, 801)]
    with _mode(K, gpu_setup, mode):
        want = _want(pool, 2, first=7)
        for _ in range(2):
            _both_forms(K, torch, gpu_setup, lists, want)


# 9
@pytest.mark.parametrize("mode", MODES)
def test_both_msm_engines(K, gpu_setup, engine_setup, mode):
    import torch
    pool = _pool(K, gpu_setup, mode)
    lists = [_pick(64, 900), _pick(77, 901)]
    with _mode(K, engine_setup, mode):
        _both_forms(K, torch, engine_setup, lists, _want(pool, 2, first=14))


# 10
def test_fk20(K, gpu_setup):
    """a settings object of its own on the cheapest table; three blobs reach its threshold of two"""
    import torch
    mode = S.MODE_CKZG
    pool = _pool(K, gpu_setup, mode)   # the MSM engine's bytes
    lists = [_pick(64, 1000), _pick(100, 1001), list(range(128))]
    want = _want(pool, 3, first=1)
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, 4, 2)
        with _mode(K, ts, mode):
            K.lib().lwkzg_profile_reset()
            K.lib().lwkzg_profile_enable(1)
            _both_forms(K, torch, ts, lists, want)
            K.lib().lwkzg_profile_enable(0)
            kernels = K.capi.profile_report()
            assert sorted(k for k in kernels if k.startswith("k_fk20")) == ["k_fk20_coeffs", "k_fk20_msm", "k_fk20_transforms"]
            assert "k_recover_mixed_solve" in kernels and "k_cells_quotients" not in kernels
            # one blob stays below the threshold: the MSM path, the same bytes
            assert K.recover_cells_and_kzg_proofs_mixed(lists[:1], _given(want[:1], lists[:1]), ts) == want[:1]
    finally:
        K.lib().lwkzg_profile_enable(0)
        K.lib().lwkzg_profile_reset()
        ts.set_cell_proof_engine(K.CELL_PROOFS_MSM)
        ts.free()
