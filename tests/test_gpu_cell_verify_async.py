"""GPU: the asynchronous cell verifier (lwkzg_cell_verifier_*). An enqueue is
lwkzg_verify_cell_kzg_proof_batch_device with the grouping on the GPU and the host's work in stream order: per batch result.ok, rc and
partials are held byte for byte against the synchronous device call and lwkzg_cell_verify_partials on the same inputs, in both modes.
Batches: one item, a repeated item, the column sidecars and their shuffle, all cells of two blobs, and a library-made batch cut at 257
and at 1025 items. Further: every single corruption, malformed inputs with their first_bad, an index of 128 decided first, the empty
batch and argument errors, that the call returns while its work is queued, stream order, the depth, two verifiers beside a
synchronous call, a setup freed under a verifier, both engines, a Lagrange-only table, and an honest batch behind a rejected one."""
import pytest

import blobs as B
import cells_spec as S
from conftest import R, SETUP_PATH
from test_gpu_cell_verify import (INF, MODES, Poly, _corruptions, _honest_batches, _mode, _partials, _sidecar, _small_batch,
                                  _x_off_the_curve)

pytestmark = pytest.mark.gpu

NONE_BAD = 0xffffffff
CAP = 1025


class _Dev:
    """a batch of items on the device"""

    def __init__(self, items):
        import torch

        def dev(data):
            return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()

        self.n = len(items)
        self.dc, self.dcell, self.dp = dev(b"".join(i[0] for i in items)), dev(b"".join(i[2] for i in items)), dev(b"".join(i[3] for i in items))
        self.di = torch.tensor([i[1] for i in items] or [0], dtype=torch.int64).cuda()
        torch.cuda.synchronize()

    def ptrs(self):
        return self.dc.data_ptr(), self.di.data_ptr(), self.dcell.data_ptr(), self.dp.data_ptr()


def _sync(K, ts, d):
    """(rc, ok) of the synchronous device call"""
    try:
        return 0, K.verify_cell_kzg_proof_batch_device(*d.ptrs(), d.n, ts)
    except K.KzgError as e:
        return e.rc, False


def _async(v, d, stream=None):
    res = v.enqueue(*d.ptrs(), d.n, stream)
    v.wait()
    assert res.state == 1 and v.pending() == 0
    return res


def _same_as_the_synchronous_call(K, ts, v, items, want_ok, name=None):
    """ok, rc and partials byte for byte; returns the result"""
    d = _Dev(items)
    res = _async(v, d)
    assert (res.rc, bool(res.ok)) == _sync(K, ts, d) == (0, want_ok), (name, res.rc, res.ok)
    assert res.first_bad == NONE_BAD and res.m == len({i[0] for i in items}), name
    assert bytes(res.partials) == _partials(K, ts, items), name
    return res


@pytest.fixture(scope="module")
def verifier(K, gpu_setup):
    v = K.CellVerifier(gpu_setup, CAP)
    yield v
    v.free()


@pytest.mark.parametrize("mode", MODES)
def test_honest_batches_equal_the_synchronous_call(K, gpu_setup, verifier, oracle, mode):
    batches = dict(_honest_batches(oracle, mode))
    batches["one_item"] = [Poly.seeded(oracle, 3000).item(77, mode)]
    assert {len(b) for b in batches.values()} == {1, 6, 48, 256}
    with _mode(K, gpu_setup, mode):
        for name, items in batches.items():
            _same_as_the_synchronous_call(K, gpu_setup, verifier, items, True, name)
        # the zero blob and a constant polynomial: commitments and proofs at infinity take part in the grouping like any other string
        gen = oracle.g1_generator_mul(12345)
        mixed = [(INF, k, bytes(2048), INF) for k in (0, 64, 127)] + [(gen, k, S.to_bytes(12345, mode) * 64, INF) for k in (1, 2, 100)]
        _same_as_the_synchronous_call(K, gpu_setup, verifier, mixed, True, "degenerate")


@pytest.fixture(scope="module")
def library_batch(K, gpu_setup):
    """the 128 cells of nine blobs with their proofs, made by the library: 1152 items per mode"""
    out = {}
    for mode in MODES:
        blobs = b"".join(B.synthetic_blob(940 + i, big_endian=mode == S.MODE_REFERENCE) for i in range(9))
        with _mode(K, gpu_setup, mode):
            comms = K.blob_to_kzg_commitment_batch(blobs, gpu_setup)
            made = K.compute_cells_and_kzg_proofs_batch(blobs, gpu_setup)
        out[mode] = [(comms[b], k, made[b][0][k], made[b][1][k]) for b in range(9) for k in range(128)]
    return out


@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("mode", MODES)
def test_library_made_batch_cut_at(K, gpu_setup, verifier, library_batch, mode, n):
    items = library_batch[mode][:n]
    with _mode(K, gpu_setup, mode):
        _same_as_the_synchronous_call(K, gpu_setup, verifier, items, True)
        # the last item's proof swapped for the first one's: the last slice of the variable-base sums
        _same_as_the_synchronous_call(K, gpu_setup, verifier, items[:-1] + [items[-1][:3] + (items[0][3],)], False)


@pytest.mark.parametrize("mode", MODES)
def test_every_single_corruption_answers_false(K, gpu_setup, verifier, oracle, mode):
    items, polys = _small_batch(oracle, mode)
    with _mode(K, gpu_setup, mode):
        for pos in (0, len(items) // 2, len(items) - 1):
            for name, bad in _corruptions(items[pos], polys, mode).items():
                _same_as_the_synchronous_call(K, gpu_setup, verifier, items[:pos] + [bad] + items[pos + 1:], False, (pos, name))


@pytest.mark.parametrize("mode", MODES)
def test_malformed_inputs_give_the_modes_code_and_first_bad(K, gpu_setup, verifier, oracle, mode):
    items, _ = _small_batch(oracle, mode)     # 12 items over 3 commitments: rows 0 1 2 0 1 2 ...
    want = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    order3 = bytes([0x80]) + bytes(47)
    c, k, cell, proof = items[4]

    def answer(batch):
        d = _Dev(batch)
        res = _async(verifier, d)
        assert (res.rc, False) == _sync(K, gpu_setup, d) and res.ok == 0
        assert bytes(res.partials) == bytes(len(res.partials))
        return res.rc, res.first_bad

    with _mode(K, gpu_setup, mode):
        for name, bad in [("proof outside the subgroup", (c, k, cell, order3)), ("proof off the curve", (c, k, cell, _x_off_the_curve())),
                          ("element equal to r", (c, k, cell[:64] + S.to_bytes(R, mode) + cell[96:], proof)),
                          ("element 2^256 - 1", (c, k, cell[:2016] + b"\xff" * 32, proof))]:
            for pos in (0, 4, len(items) - 1):
                assert answer(items[:pos] + [bad] + items[pos + 1:]) == (want, pos), (name, pos)
        # a commitment outside the subgroup, as a row of its own, counts where it is first seen
        for pos in (0, 4, len(items) - 1):
            assert answer(items[:pos] + [(order3, k, cell, proof)] + items[pos + 1:]) == (want, pos)
        # the same bad commitment at 5 and 9, a bad proof at 7: the commitment's first item is the lowest at fault
        batch = list(items)
        for pos in (5, 9):
            batch[pos] = (order3,) + batch[pos][1:]
        batch[7] = batch[7][:3] + (order3,)
        assert answer(batch) == (want, 5)
        batch[3] = batch[3][:3] + (_x_off_the_curve(),)
        assert answer(batch) == (want, 3)
        # an index of 128 is decided first, in both modes, whatever else is wrong; the lowest such item
        batch[8] = (batch[8][0], 128) + batch[8][2:]
        assert answer(batch) == (K.C_KZG_BADARGS, 8)
        batch[2] = (batch[2][0], (1 << 63) - 1) + batch[2][2:]
        assert answer(batch) == (K.C_KZG_BADARGS, 2)
        assert answer(items[:11] + [(items[11][0], 128) + items[11][2:]]) == (K.C_KZG_BADARGS, 11)
        # r - 1 is a value like any other, and the verifier is none the worse: an honest batch behind the rejected ones
        _same_as_the_synchronous_call(K, gpu_setup, verifier, items[:4] + [(c, k, cell[:64] + S.to_bytes(R - 1, mode) + cell[96:], proof)] + items[5:],
                                      False)
        _same_as_the_synchronous_call(K, gpu_setup, verifier, items, True)


@pytest.mark.parametrize("mode", MODES)
def test_a_rejected_batch_leaves_nothing_stale_behind(K, gpu_setup, oracle, mode):
    """a fresh verifier whose FIRST call is rejected (nothing behind r has ever run on its buffers), then honest batches of another
    size and of the same size, back to back without a wait in between"""
    items = _sidecar(oracle, mode)
    rejected = items[:20] + [(items[20][0], 500) + items[20][2:]] + items[21:]
    v = K.CellVerifier(gpu_setup, 64)
    try:
        with _mode(K, gpu_setup, mode):
            d_bad, d_small, d_all = _Dev(rejected), _Dev(items[:7]), _Dev(items)
            results = [v.enqueue(*d.ptrs(), d.n) for d in (d_bad, d_small, d_bad, d_all)]
            v.wait()
            assert [(r.state, r.rc, r.ok, r.first_bad) for r in results] == [(1, K.C_KZG_BADARGS, 0, 20), (1, 0, 1, NONE_BAD)] * 2
            assert bytes(results[1].partials) == _partials(K, gpu_setup, items[:7])
            assert bytes(results[3].partials) == _partials(K, gpu_setup, items)
    finally:
        v.free()


def _long_work(torch, stream):
    """known-long work on `stream`: a spin of ~300 ms where torch has one (calibrated first), else large matrix products"""
    if hasattr(torch.cuda, "_sleep"):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(2000000)
        t1.record(stream)
        t1.synchronize()
        ms = t0.elapsed_time(t1)
        if 0.01 < ms < 300:
            with torch.cuda.stream(stream):
                torch.cuda._sleep(int(2000000 * 300 / ms))
            return
    with torch.cuda.stream(stream):
        a = torch.randn(8192, 8192, device="cuda")
        for _ in range(40):
            a = (a @ a).clamp_(-1, 1)
    stream._keep = a


def test_enqueue_returns_without_waiting_and_the_verdict_is_in_stream_order(K, gpu_setup, verifier, oracle):
    """long work queued ahead on the caller's stream: enqueue returns with the result pending and the stream busy. Work enqueued
    BEHIND the call sees the verdict: a proof overwritten on the stream after the first enqueue does not reach it, and reaches the second"""
    import torch
    items = _sidecar(oracle, S.MODE_REFERENCE)
    d = _Dev(items)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _mode(K, gpu_setup, S.MODE_REFERENCE):
        _long_work(torch, st)
        first = verifier.enqueue(*d.ptrs(), d.n, st.cuda_stream)
        state, pending, drained = first.state, verifier.pending(), st.query()
        with torch.cuda.stream(st):
            d.dp[48 * 17:48 * 18] = d.dp[48 * 3:48 * 4].clone()   # ordered behind the first verdict: enqueue joins its end into the stream
        second = verifier.enqueue(*d.ptrs(), d.n, st.cuda_stream)
        assert (state, pending, drained) == (0, 1, False)
        verifier.wait()
    assert (first.state, first.rc, first.ok) == (1, 0, 1) and (second.state, second.rc, second.ok) == (1, 0, 0)
    st.synchronize()


def test_depth_six_enqueues_back_to_back(K, gpu_setup, verifier, oracle):
    items = _sidecar(oracle, S.MODE_REFERENCE)
    good, bad = _Dev(items), _Dev(items[:20] + [items[20][:3] + (items[21][3],)] + items[21:])
    results, seen = [], []
    with _mode(K, gpu_setup, S.MODE_REFERENCE):
        for q in range(6):
            d = bad if q & 1 else good
            results.append(verifier.enqueue(*d.ptrs(), d.n))
            seen.append(verifier.pending())
        verifier.wait()
    assert max(seen) <= K.VERIFIER_DEPTH and min(seen) >= 0, seen
    assert [(r.state, r.rc, r.ok) for r in results] == [(1, 0, 1), (1, 0, 0)] * 3


def test_two_verifiers_on_two_streams_beside_a_synchronous_call(K, gpu_setup, verifier, oracle, library_batch):
    import torch
    mode = S.MODE_REFERENCE
    big = library_batch[mode]
    gpu_setup.reserve(8, caller_streams=2)
    second = K.CellVerifier(gpu_setup, 300)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        d1, d3 = _Dev(big[:257]), _Dev(big[300:557])
        d2 = _Dev(big[600:700] + [big[700][:3] + (big[701][3],)] + big[701:857])
        small = _Dev(_sidecar(oracle, mode))
        with _mode(K, gpu_setup, mode):
            r1 = verifier.enqueue(*d1.ptrs(), d1.n, s1.cuda_stream)
            sync_ok = K.verify_cell_kzg_proof_batch_device(*small.ptrs(), small.n, gpu_setup)
            r2 = second.enqueue(*d2.ptrs(), d2.n, s2.cuda_stream)
            r3 = verifier.enqueue(*d3.ptrs(), d3.n, s1.cuda_stream)
            verifier.wait()
            second.wait()
        assert sync_ok is True
        assert [(r.state, r.rc, r.ok, r.m) for r in (r1, r2, r3)] == [(1, 0, 1, 3), (1, 0, 0, 3), (1, 0, 1, 3)]
        torch.cuda.synchronize()
    finally:
        second.free()


def test_empty_batch_and_argument_errors_complete_on_the_spot(K, gpu_setup, verifier, oracle):
    for mode in MODES:
        with _mode(K, gpu_setup, mode):
            res = verifier.enqueue(None, None, None, None, 0)
            assert (res.state, res.rc, res.ok, res.first_bad, verifier.pending()) == (1, 0, 1, NONE_BAD, 0)
    d = _Dev(_sidecar(oracle, S.MODE_REFERENCE))
    small = K.CellVerifier(gpu_setup, 8)
    try:
        with pytest.raises(K.KzgError) as e:
            small.enqueue(*d.ptrs(), 9)
        assert e.value.rc == K.C_KZG_BADARGS
        assert (e.value.result.state, e.value.result.rc, e.value.result.ok) == (1, K.C_KZG_BADARGS, 0)
        for missing in range(4):
            ptrs = list(d.ptrs())
            ptrs[missing] = None
            with pytest.raises(K.KzgError) as e:
                small.enqueue(*ptrs, 3)
            assert e.value.rc == K.C_KZG_BADARGS and e.value.result.state == 1 and e.value.result.rc == K.C_KZG_BADARGS
        assert small.pending() == 0
        with pytest.raises(K.KzgError) as e:
            K.CellVerifier(gpu_setup, 0)
        assert e.value.rc == K.C_KZG_BADARGS
        with _mode(K, gpu_setup, S.MODE_REFERENCE):   # and the small verifier works: a batch that fills it
            res = small.enqueue(*d.ptrs(), 8)
            small.wait()
            assert (res.state, res.rc, res.ok) == (1, 0, 1)
    finally:
        small.free()


def test_setup_freed_under_a_verifier(K, oracle):
    """free_trusted_setup waits for the cell verifier's call in flight; the verifier then refuses, and is still freed cleanly"""
    d = _Dev(_sidecar(oracle, S.MODE_REFERENCE))
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    ts.set_mode(K.MODE_REFERENCE)
    v = K.CellVerifier(ts, 64)
    res = v.enqueue(*d.ptrs(), d.n)
    ts.free()
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 1, NONE_BAD)
    with pytest.raises(K.KzgError) as e:
        v.enqueue(*d.ptrs(), d.n)
    assert e.value.rc == K.C_KZG_BADARGS and e.value.result.state == 1
    v.free()
    assert v.pending() == -1


@pytest.mark.parametrize("mode", MODES)
def test_both_engines(K, engine_setup, oracle, mode):
    items = _sidecar(oracle, mode)
    v = K.CellVerifier(engine_setup, 64)
    try:
        with _mode(K, engine_setup, mode):
            _same_as_the_synchronous_call(K, engine_setup, v, items, True)
            _same_as_the_synchronous_call(K, engine_setup, v, items[:-1] + [items[-1][:3] + (items[0][3],)], False)
    finally:
        v.free()


def test_lagrange_only_table_in_ckzg_mode(K, oracle):
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        ts.set_mode(K.MODE_CKZG)
        ts.enable_direct_table_forms(10, 2)
        assert ts.direct_table_forms() == 2
        items = _sidecar(oracle, S.MODE_CKZG)
        v = K.CellVerifier(ts, 64)
        try:
            _same_as_the_synchronous_call(K, ts, v, items, True)
            _same_as_the_synchronous_call(K, ts, v, items[1:] + [items[0][:2] + (items[1][2], items[0][3])], False)
        finally:
            v.free()
    finally:
        ts.free()
