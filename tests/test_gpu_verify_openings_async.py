"""GPU: lwkzg_verifier_enqueue_openings -- lwkzg_verify_kzg_proof_batch_device without a parked host thread, on the blob batch's
verifier (DESIGN.md sections 4m, 4p). Checked here: rc, ok, first_bad, r and partial against the synchronous call and its hook at
n = 1, 65 and 1025; a rejected batch (the lowest index, a zero partial); blob and opening calls interleaved on one verifier; five
calls back to back; what completes on the spot; and stream order behind a call."""
import pytest

import blobs as B
import openings_cases as OC

pytestmark = pytest.mark.gpu

NONE_BAD = 0xffffffff
CAP = 1025


def _dev(torch, data):
    return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()


class _Dev:
    def __init__(self, torch, items):
        self.n = len(items)
        self.bufs = [_dev(torch, col) for col in OC.columns(items)]
        torch.cuda.synchronize()

    def ptrs(self):
        return [b.data_ptr() for b in self.bufs]


@pytest.fixture(scope="module")
def verifier(K, gpu_setup):
    v = K.Verifier(gpu_setup, CAP)
    yield v
    v.free()


def _enqueue(torch, v, d, stream=None):
    torch.cuda.synchronize()
    res = v.enqueue_openings(*d.ptrs(), d.n, stream)
    v.wait()
    assert res.state == 1 and v.pending() == 0
    return res


def _sync(K, d, ts):
    try:
        return 0, K.verify_kzg_proof_batch_device(*d.ptrs(), d.n, ts)
    except K.KzgError as e:
        return e.rc, False


@pytest.mark.parametrize("n", [1, 65, 1025])
@pytest.mark.parametrize("mode_name", ["reference", "ckzg", "eth"])
def test_result_equals_the_synchronous_call_and_its_hook(K, gpu_setup, verifier, mode_name, n):
    import torch
    mode = {"reference": K.MODE_REFERENCE, "ckzg": K.MODE_CKZG, "eth": K.MODE_ETH}[mode_name]
    code = OC.mode_code(K, mode)
    with OC.Mode(gpu_setup, mode):
        honest = OC.draw(OC.pool(K, gpu_setup, mode), n, 1300 + n)
        tampered = list(honest)
        tampered[n // 2] = OC.tamper_y(K, mode, honest[n // 2])
        for items, ok in ((honest, True), (tampered, False)):
            d = _Dev(torch, items)
            res = _enqueue(torch, verifier, d)
            assert (res.rc, res.ok, res.first_bad) == (0, int(ok), NONE_BAD), (n, res.rc, res.ok, res.first_bad)
            assert _sync(K, d, gpu_setup) == (0, ok)
            r, partial = K.verify_kzg_proof_batch_partial(*OC.columns(items), gpu_setup)
            assert bytes(res.r) == r and bytes(res.partial) == partial
            assert r == K.batch_challenge_host(b"".join(b"".join(t) for t in items), n, mode)
        # a rejected batch: the lowest index, the mode's code, a zero partial; nothing behind r ran
        order = OC.order_of(K, mode)
        bad = list(honest)
        lo, hi = (0, 0) if n == 1 else (n // 3, n - 1)
        c, z, y, p = bad[hi]
        bad[hi] = (c, z, y, bytes(48))                       # an invalid proof encoding
        c, z, y, p = bad[lo]
        bad[lo] = (bytes([c[0] & 0x7f]) + c[1:], z, y, p)    # an invalid commitment encoding
        d = _Dev(torch, bad)
        res = _enqueue(torch, verifier, d)
        assert (res.rc, res.ok, res.first_bad) == (code, 0, lo)
        assert bytes(res.partial) == bytes(328) and bytes(res.r) == bytes(32)
        assert _sync(K, d, gpu_setup) == (code, False)
        if mode != K.MODE_REFERENCE:   # a scalar that is not below r, behind valid points
            bad = list(honest)
            c, z, y, p = bad[n - 1]
            bad[n - 1] = (c, z, OC.R.to_bytes(32, order), p)
            res = _enqueue(torch, verifier, _Dev(torch, bad))
            assert (res.rc, res.ok, res.first_bad) == (code, 0, n - 1)


def test_blob_and_opening_calls_interleaved(K, gpu_setup, verifier):
    import torch
    mode = K.MODE_REFERENCE
    n = 65
    with OC.Mode(gpu_setup, mode):
        data = B.synthetic_batch(58000, n)
        cj = b"".join(K.blob_to_kzg_commitment_batch(data, gpu_setup))
        pj = b"".join(K.compute_blob_kzg_proof_batch(data, cj, gpu_setup))
        db, dc, dp = _dev(torch, data), _dev(torch, cj), _dev(torch, pj)
        dp_bad = _dev(torch, pj[48:96] + pj[48:])
        honest = OC.draw(OC.pool(K, gpu_setup, mode), 300, 61)
        tampered = list(honest)
        tampered[299] = OC.tamper_y(K, mode, honest[299])
        good, bad = _Dev(torch, honest), _Dev(torch, tampered)
        torch.cuda.synchronize()
        results, seen = [], []
        for q in range(3):
            results.append(verifier.enqueue(db.data_ptr(), dc.data_ptr(), (dp_bad if q == 1 else dp).data_ptr(), n))
            seen.append(verifier.pending())
            results.append(verifier.enqueue_openings(*(bad if q == 2 else good).ptrs(), 300))
            seen.append(verifier.pending())
        verifier.wait()
        assert [(r.state, r.rc, r.ok, r.first_bad) for r in results] == [(1, 0, k, NONE_BAD) for k in (1, 1, 0, 1, 1, 0)]
        assert max(seen) <= K.VERIFIER_DEPTH
        # in order: each result's r is its own batch's
        r_open, _ = K.verify_kzg_proof_batch_partial(*OC.columns(honest), gpu_setup)
        assert bytes(results[1].r) == r_open == bytes(results[3].r) and bytes(results[5].r) != r_open
        assert bytes(results[0].r) == bytes(results[4].r) != bytes(results[2].r)


def test_five_calls_back_to_back(K, gpu_setup, verifier):
    """LWKZG_VERIFIER_DEPTH calls are in flight at most; the fifth waits for the oldest, and none is lost"""
    import torch
    mode = K.MODE_CKZG
    with OC.Mode(gpu_setup, mode):
        honest = OC.draw(OC.pool(K, gpu_setup, mode), 257, 63)
        tampered = list(honest)
        tampered[0] = OC.tamper_y(K, mode, honest[0])
        good, bad = _Dev(torch, honest), _Dev(torch, tampered)
        results, seen = [], []
        for q in range(5):
            results.append(verifier.enqueue_openings(*(bad if q & 1 else good).ptrs(), 257))
            seen.append(verifier.pending())
        verifier.wait()
        assert max(seen) <= K.VERIFIER_DEPTH and min(seen) >= 0, seen
        assert [(r.state, r.rc, r.ok) for r in results] == [(1, 0, 1), (1, 0, 0), (1, 0, 1), (1, 0, 0), (1, 0, 1)]


def test_what_completes_on_the_spot(K, gpu_setup, verifier):
    import torch
    buf = _dev(torch, bytes(1024))
    torch.cuda.synchronize()
    p = buf.data_ptr()
    for mode, empty in ((K.MODE_REFERENCE, 0), (K.MODE_CKZG, 1), (K.MODE_ETH, 1)):
        with OC.Mode(gpu_setup, mode):
            res = verifier.enqueue_openings(None, None, None, None, 0)
            assert (res.state, res.rc, res.ok, verifier.pending()) == (1, 0, empty, 0)
    small = K.Verifier(gpu_setup, 8)
    try:
        for args in ((p, p + 64, p + 128, p + 192, 9),        # above the capacity
                     (p, None, p + 128, p + 192, 3),           # a NULL input
                     (p, p + 64, p + 128 + 4, p + 192, 3)):    # a misaligned input
            with pytest.raises(K.KzgError) as e:
                small.enqueue_openings(*args)
            assert e.value.rc == K.C_KZG_BADARGS
            assert (e.value.result.state, e.value.result.rc, e.value.result.ok) == (1, K.C_KZG_BADARGS, 0)
        assert small.pending() == 0
    finally:
        small.free()


def test_work_behind_a_call_on_the_stream_sees_the_verdict(K, gpu_setup, verifier):
    """the columns are produced on a caller stream; an event recorded on that stream BEHIND the call has passed only once the
    result is complete (no verifier.wait() in between)"""
    import torch
    mode = K.MODE_REFERENCE
    n = 300
    with OC.Mode(gpu_setup, mode):
        items = OC.draw(OC.pool(K, gpu_setup, mode), n, 67)
        src = [_dev(torch, col) for col in OC.columns(items)]
        dst = [torch.zeros_like(s) for s in src]
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for d, s in zip(dst, src):
                d.copy_(s, non_blocking=True)
            res = verifier.enqueue_openings(*[d.data_ptr() for d in dst], n, st.cuda_stream)
            done = torch.cuda.Event()
            done.record(st)
        done.synchronize()
        assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 1, NONE_BAD)
        verifier.wait()
