"""GPU: the asynchronous batch verifier (lwkzg_verifier_*). An enqueue is
lwkzg_verify_blob_kzg_proof_batch_device split where that call first waits: same verdicts, return codes and empty-batch rule
(/root/reference/src/lib.rs:525-614, 639-692), written to a LwkzgVerifyResult in stream order instead of a host bool. Checked here:
the verdicts and codes against the synchronous device call at the lane, wave and workgroup edges of k_verify_ysum (1, 2, 3, 64, 65,
257, 300) and one chunk + 1 (1025); result.partial and result.r byte for byte against the sharded form's host walk; that the call
returns while its work is still queued; stream order; the depth of one verifier; two verifiers on two streams beside a synchronous
call; the empty batch; argument errors; a setup freed under a verifier with a call in flight; one verifier sent to the settings'
second context and back by construction; and the experiment arm without the bucket MSM, where enqueue completes the result itself."""
import random

import pytest

import blobs as B
from conftest import R, SETUP_PATH

pytestmark = pytest.mark.gpu

BLOB = B.BYTES_PER_BLOB
N_REF = 1025
NONE_BAD = 0xffffffff


def _dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


class _Batch:
    """an honest batch on the device (blobs, commitments, proofs), its host copies, and one more valid blob / point to swap in"""

    def __init__(self, K, torch, ts, data, n, spare_blob, spare_point):
        self.n, self.data = n, data
        self.cj = b"".join(K.blob_to_kzg_commitment_batch(data, ts))
        self.pj = b"".join(K.compute_blob_kzg_proof_batch(data, self.cj, ts))
        self.db, self.dc, self.dp = _dev(torch, data), _dev(torch, self.cj), _dev(torch, self.pj)
        self.spare_blob, self.spare_point = _dev(torch, spare_blob), spare_point
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def ref_batch(K, gpu_setup, oracle):
    """1025 reference-mode blobs, computed once: every test below verifies prefixes (or slices) of it. A zero blob and a constant
    blob (commitment and proof at infinity / proof at infinity) sit at 1 and 2, so they take part whenever n > 2."""
    import torch
    K.set_mode(K.MODE_REFERENCE)
    blobs = [B.synthetic_blob(77000 + i) for i in range(N_REF)]
    blobs[1] = bytes(BLOB)
    const = bytearray(BLOB)
    const[31] = 5
    blobs[2] = bytes(const)
    return _Batch(K, torch, gpu_setup, b"".join(blobs), N_REF, B.synthetic_blob(99300), oracle.g1_generator_mul(424243))


@pytest.fixture(scope="module")
def ckzg_batch(K, gpu_setup, oracle):
    import torch
    K.set_mode(K.MODE_CKZG)
    try:
        return _Batch(K, torch, gpu_setup, B.synthetic_batch(78000, 300, big_endian=False), 300,
                      B.synthetic_blob(99301, big_endian=False), oracle.g1_generator_mul(424244))
    finally:
        K.set_mode(K.MODE_REFERENCE)


@pytest.fixture(scope="module")
def verifier(K, gpu_setup):
    v = K.Verifier(gpu_setup, N_REF)
    yield v
    v.free()


def _sync(K, torch, b, dc, dp, n, ts):
    """(rc, ok) of the synchronous device call"""
    torch.cuda.synchronize()
    try:
        return 0, K.verify_blob_kzg_proof_batch_device(b.db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, ts)
    except K.KzgError as e:
        return e.rc, False


def _async(torch, v, b, dc, dp, n, stream=None):
    torch.cuda.synchronize()
    res = v.enqueue(b.db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, stream)
    v.wait()
    assert res.state == 1 and v.pending() == 0
    return res


def _swap(torch, buf, i, piece):
    return _dev(torch, buf[:48 * i] + piece + buf[48 * i + 48:])


def _verdicts_and_bytes(K, torch, ts, v, b, n, mode, bad_code):
    from lambdaworks_kzg_amd import capi
    rnd = random.Random(8100 + n)
    # honest: the verdict, and r and the partial sums byte for byte against the sharded form (whose sum r^i y_i is the host's walk)
    res = _async(torch, v, b, b.dc, b.dp, n)
    assert (res.rc, res.ok, res.first_bad) == (0, 1, NONE_BAD), (n, res.rc, res.ok, res.first_bad)
    assert _sync(K, torch, b, b.dc, b.dp, n, ts) == (0, True)
    shard = capi.VerifyShard.from_device(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), n, ts)
    try:
        assert bytes(res.partial) == shard.partial(shard.records, n, 0), n
        assert bytes(res.r) == K.batch_challenge_host(shard.records, n, mode), n
    finally:
        shard.free()
    # one proof, one commitment, one blob swapped for another valid one
    i, j, k = rnd.randrange(n), rnd.randrange(n), rnd.randrange(n)
    for dc, dp in ((b.dc, _swap(torch, b.pj[:48 * n], i, b.spare_point)), (_swap(torch, b.cj[:48 * n], j, b.spare_point), b.dp)):
        res = _async(torch, v, b, dc, dp, n)
        assert (res.rc, res.ok, res.first_bad) == (0, 0, NONE_BAD), n
        assert _sync(K, torch, b, dc, dp, n, ts) == (0, False)
    saved = b.db[k * BLOB:(k + 1) * BLOB].clone()
    b.db[k * BLOB:(k + 1) * BLOB] = b.spare_blob
    try:
        res = _async(torch, v, b, b.dc, b.dp, n)
        assert (res.rc, res.ok, res.first_bad) == (0, 0, NONE_BAD), n
        assert _sync(K, torch, b, b.dc, b.dp, n, ts) == (0, False)
    finally:
        b.db[k * BLOB:(k + 1) * BLOB] = saved
        torch.cuda.synchronize()
    # an invalid point is an answer of the RESULT (the mode's code, the index), not of the call: three encodings
    cj, pj = b.cj[:48 * n], b.pj[:48 * n]
    for badc, badp, where in ((bytes(48) + cj[48:], pj, 0), (cj, pj[:-48] + bytes(48), n - 1), (bytes([cj[0] & 0x7f]) + cj[1:], pj, 0)):
        dc, dp = _dev(torch, badc), _dev(torch, badp)
        res = _async(torch, v, b, dc, dp, n)
        assert (res.rc, res.ok, res.first_bad) == (bad_code, 0, where), (n, res.rc, res.ok, res.first_bad)
        assert _sync(K, torch, b, dc, dp, n, ts) == (bad_code, False)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257, 300, 1025])
def test_verdicts_codes_and_bytes_equal_the_synchronous_call(K, gpu_setup, verifier, ref_batch, n):
    import torch
    _verdicts_and_bytes(K, torch, gpu_setup, verifier, ref_batch, n, K.MODE_REFERENCE, K.C_KZG_ERROR)


@pytest.mark.parametrize("n", [3, 300])
def test_ckzg_mode_verdicts_codes_and_bytes(K, gpu_setup, verifier, ckzg_batch, n):
    """c-kzg mode (little-endian blobs on the Lagrange form): the same, invalid points are C_KZG_BADARGS, and ONE element >= r
    anywhere in the batch is C_KZG_BADARGS at that blob's index"""
    import torch
    K.set_mode(K.MODE_CKZG)
    try:
        b = ckzg_batch
        _verdicts_and_bytes(K, torch, gpu_setup, verifier, b, n, K.MODE_CKZG, K.C_KZG_BADARGS)
        for where in (0, n - 1):
            off = where * BLOB + 32 * 1234
            saved = b.db[off:off + 32].clone()
            b.db[off:off + 32] = _dev(torch, R.to_bytes(32, "little"))
            try:
                res = _async(torch, verifier, b, b.dc, b.dp, n)
                assert (res.rc, res.ok, res.first_bad) == (K.C_KZG_BADARGS, 0, where)
                assert _sync(K, torch, b, b.dc, b.dp, n, gpu_setup) == (K.C_KZG_BADARGS, False)
            finally:
                b.db[off:off + 32] = saved
                torch.cuda.synchronize()
    finally:
        K.set_mode(K.MODE_REFERENCE)


def _long_work(torch, capi, ts, b, stream):
    """known-long work on `stream`: a spin of ~300 ms where torch has one (calibrated first: its unit is the device's counter),
    else commitments and proofs of the whole batch, three times"""
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
    out_c = torch.empty(48 * b.n, dtype=torch.uint8, device="cuda")
    out_p = torch.empty(48 * b.n, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        capi.commit_and_prove_batch_device(out_c.data_ptr(), out_p.data_ptr(), b.db.data_ptr(), b.n, ts, stream.cuda_stream)
    stream._keep = (out_c, out_p)


def test_enqueue_returns_without_waiting(K, gpu_setup, verifier, ref_batch):
    import torch
    from lambdaworks_kzg_amd import capi
    b, n = ref_batch, 300
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    _long_work(torch, capi, gpu_setup, b, st)
    res = verifier.enqueue(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), n, st.cuda_stream)
    state, pending, drained = res.state, verifier.pending(), st.query()
    assert (state, pending, drained) == (0, 1, False)
    verifier.wait()
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 1, NONE_BAD)
    st.synchronize()


def test_stream_order(K, gpu_setup, verifier):
    """commitments and proofs computed on a caller stream and enqueued at once; one proof overwritten ON the stream and enqueued
    again; no synchronisation in between: True, then False"""
    import torch
    from lambdaworks_kzg_amd import capi
    n = 300
    data = B.synthetic_batch(91500, n)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        db = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(non_blocking=False)
        dc = torch.empty(48 * n, dtype=torch.uint8, device="cuda")
        dp = torch.empty(48 * n, dtype=torch.uint8, device="cuda")
        capi.commit_and_prove_batch_device(dc.data_ptr(), dp.data_ptr(), db.data_ptr(), n, gpu_setup, st.cuda_stream)
        first = verifier.enqueue(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, st.cuda_stream)
        dp[48 * 17:48 * 18] = dp[48 * 3:48 * 4].clone()   # ordered behind the first verdict: enqueue joins its end into the stream
        second = verifier.enqueue(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, st.cuda_stream)
    verifier.wait()
    assert (first.state, first.rc, first.ok) == (1, 0, 1)
    assert (second.state, second.rc, second.ok) == (1, 0, 0)
    torch.cuda.synchronize()


def test_depth_six_enqueues_back_to_back(K, gpu_setup, verifier, ref_batch):
    import torch
    b, n = ref_batch, 65
    tampered = _swap(torch, b.pj[:48 * n], 40, b.spare_point)
    torch.cuda.synchronize()
    results, seen = [], []
    for q in range(6):
        results.append(verifier.enqueue(b.db.data_ptr(), b.dc.data_ptr(), (tampered if q & 1 else b.dp).data_ptr(), n))
        seen.append(verifier.pending())
    verifier.wait()
    assert max(seen) <= K.VERIFIER_DEPTH and min(seen) >= 0, seen
    assert [(r.state, r.rc, r.ok) for r in results] == [(1, 0, 1), (1, 0, 0)] * 3


def test_two_verifiers_on_two_streams_beside_a_synchronous_call(K, gpu_setup, verifier, ref_batch):
    import torch
    b, n = ref_batch, 257
    gpu_setup.reserve(n, caller_streams=2)
    second = K.Verifier(gpu_setup, n)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        off = 300   # the other batch: blobs 300 .. 556, with one proof swapped
        tampered = _swap(torch, b.pj[48 * off:48 * (off + n)], 100, b.spare_point)
        torch.cuda.synchronize()
        r1 = verifier.enqueue(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), n, s1.cuda_stream)
        sync_ok = K.verify_blob_kzg_proof_batch_device(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), 65, gpu_setup)
        r2 = second.enqueue(b.db.data_ptr() + off * BLOB, b.dc.data_ptr() + 48 * off, tampered.data_ptr(), n, s2.cuda_stream)
        r3 = verifier.enqueue(b.db.data_ptr() + off * BLOB, b.dc.data_ptr() + 48 * off, b.dp.data_ptr() + 48 * off, n, s1.cuda_stream)
        verifier.wait()
        second.wait()
        assert sync_ok is True
        assert [(r.state, r.rc, r.ok) for r in (r1, r2, r3)] == [(1, 0, 1), (1, 0, 0), (1, 0, 1)]
        torch.cuda.synchronize()
    finally:
        second.free()


def test_empty_batch_both_modes_completes_on_the_spot(K, gpu_setup, verifier):
    res = verifier.enqueue(None, None, None, 0)
    assert (res.state, res.rc, res.ok, verifier.pending()) == (1, 0, 0, 0)       # lib.rs:538-543
    K.set_mode(K.MODE_CKZG)
    try:
        res = verifier.enqueue(None, None, None, 0)
        assert (res.state, res.rc, res.ok, verifier.pending()) == (1, 0, 1, 0)   # c-kzg vector a271b78b8e869d69
    finally:
        K.set_mode(K.MODE_REFERENCE)


def test_argument_errors_complete_the_result(K, gpu_setup, verifier, ref_batch):
    b = ref_batch
    small = K.Verifier(gpu_setup, 8)
    try:
        with pytest.raises(K.KzgError) as e:
            small.enqueue(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), 9)
        assert e.value.rc == K.C_KZG_BADARGS
        assert (e.value.result.state, e.value.result.rc, e.value.result.ok) == (1, K.C_KZG_BADARGS, 0)
        with pytest.raises(K.KzgError) as e:
            small.enqueue(None, b.dc.data_ptr(), b.dp.data_ptr(), 3)
        assert e.value.rc == K.C_KZG_BADARGS and e.value.result.state == 1 and e.value.result.rc == K.C_KZG_BADARGS
        assert small.pending() == 0
        with pytest.raises(K.KzgError) as e:
            K.Verifier(gpu_setup, 0)
        assert e.value.rc == K.C_KZG_BADARGS
    finally:
        small.free()


def test_setup_freed_under_a_verifier(K, ref_batch):
    """free_trusted_setup waits for the verifier's call in flight; the verifier then refuses, and is still freed cleanly"""
    import torch
    b, n = ref_batch, 300
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    v = K.Verifier(ts, n)
    torch.cuda.synchronize()
    res = v.enqueue(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), n)
    ts.free()
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 1, NONE_BAD)
    with pytest.raises(K.KzgError) as e:
        v.enqueue(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), n)
    assert e.value.rc == K.C_KZG_BADARGS and e.value.result.state == 1
    v.free()
    assert v.pending() == -1


def test_second_stream_lands_on_the_twin_and_the_next_call_comes_back(K, gpu_setup, ref_batch):
    """one verifier across the settings' two contexts, by construction rather than by timing: commitments and proofs of 1025 blobs on
    s1 leave the primary's workspace busy and last used by s1, so an enqueue on s2 goes to the twin (pick_ctx); once that call is
    complete an enqueue on s1 goes to the primary (its workspace's last user) and waits for the verifier's scratch by its last_done
    event; then the twin again. Each verdict is its own batch's."""
    import torch
    from lambdaworks_kzg_amd import capi
    b, n = ref_batch, 300
    gpu_setup.reserve(N_REF, caller_streams=2)
    v = K.Verifier(gpu_setup, n)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        out_c = torch.empty(48 * b.n, dtype=torch.uint8, device="cuda")
        out_p = torch.empty(48 * b.n, dtype=torch.uint8, device="cuda")
        tampered = _swap(torch, b.pj[:48 * n], 200, b.spare_point)
        torch.cuda.synchronize()

        def busy_primary():
            capi.commit_and_prove_batch_device(out_c.data_ptr(), out_p.data_ptr(), b.db.data_ptr(), b.n, gpu_setup, s1.cuda_stream)

        busy_primary()
        r1 = v.enqueue(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), n, s2.cuda_stream)            # twin
        v.wait()
        r2 = v.enqueue(b.db.data_ptr(), b.dc.data_ptr(), tampered.data_ptr(), n, s1.cuda_stream)        # primary, behind last_done
        v.wait()
        busy_primary()
        r3 = v.enqueue(b.db.data_ptr(), b.dc.data_ptr(), b.dp.data_ptr(), n, s2.cuda_stream)            # twin again
        v.wait()
        assert [(r.state, r.rc, r.ok) for r in (r1, r2, r3)] == [(1, 0, 1), (1, 0, 0), (1, 0, 1)]
        torch.cuda.synchronize()
        assert bytes(out_c.cpu().numpy().tobytes()) == b.cj and bytes(out_p.cpu().numpy().tobytes()) == b.pj
    finally:
        v.free()


_FALLBACK = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "golden"))
import torch
import blobs as B
import lambdaworks_kzg_amd as K
from lambdaworks_kzg_amd import capi
ts = K.TrustedSetup.from_file(os.path.join(sys.argv[1], "tests", "golden", "trusted_setup.txt"))
n = 5
data = B.synthetic_batch(93000, n)
cj = b"".join(K.blob_to_kzg_commitment_batch(data, ts)); pj = b"".join(K.compute_blob_kzg_proof_batch(data, cj, ts))
dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
db, dc, dp, bad = dev(data), dev(cj), dev(pj), dev(pj[48:96] + pj[48:])
torch.cuda.synchronize()
v = K.Verifier(ts, n)
r1 = v.enqueue(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n)
s1 = (r1.state, r1.rc, r1.ok, v.pending())          # complete when enqueue returns
r2 = v.enqueue(db.data_ptr(), dc.data_ptr(), bad.data_ptr(), n)
s2 = (r2.state, r2.rc, r2.ok, v.pending())
r3 = v.enqueue(db.data_ptr(), dev(bytes(48) + cj[48:]).data_ptr(), dp.data_ptr(), n)
s3 = (r3.state, r3.rc, r3.ok)
sh = capi.VerifyShard.from_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, ts)
same = bytes(r1.partial) == sh.partial(sh.records, n, 0) and bytes(r1.r) == K.batch_challenge_host(sh.records, n, K.MODE_REFERENCE)
sh.free(); v.free(); ts.free()
print("fallback", s1, s2, s3, same)
"""


def test_the_experiment_arm_without_the_bucket_msm_completes_inside_enqueue():
    """LWKZG_EXPERIMENTAL=1 LWKZG_VERIFY_MSM=0 (knobs are read once per process: a process of its own): enqueue runs the synchronous
    path and the result is complete when it returns -- same verdicts, code, r and partial"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, LWKZG_EXPERIMENTAL="1", LWKZG_VERIFY_MSM="0")
    out = subprocess.run([sys.executable, "-c", _FALLBACK, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "fallback (1, 0, 1, 0) (1, 0, 0, 0) (1, 2, 0) True" in out.stdout, out.stdout[-2000:]
