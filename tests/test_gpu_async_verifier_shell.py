"""GPU: what the blob verifier and the cell verifier that do not block share (csrc/async_verifier.h; DESIGN.md sections 4m, 4n), where
the two kinds meet: a handle of one kind at the other kind's entry points, and one trusted setup freed under a call in flight of each
kind (ctx_destroy drains both through the one registry). Shapes: 3 blobs; the cell tests' 48-item sidecar on a 64-item verifier."""
import ctypes as C

import pytest

import blobs as B
import cells_spec as S
from conftest import SETUP_PATH
from test_gpu_cell_verify import _mode, _sidecar
from test_gpu_cell_verify_async import _Dev

pytestmark = pytest.mark.gpu

NONE_BAD = 0xffffffff
N_BLOBS = 3


@pytest.fixture(scope="module")
def blob_ptrs(K, gpu_setup):
    """three honest reference-mode blobs with their commitments and proofs on the device: the pointers, and what keeps them alive"""
    import torch
    K.set_mode(K.MODE_REFERENCE)
    data = B.synthetic_batch(95000, N_BLOBS)
    cj = b"".join(K.blob_to_kzg_commitment_batch(data, gpu_setup))
    pj = b"".join(K.compute_blob_kzg_proof_batch(data, cj, gpu_setup))
    keep = [torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda() for x in (data, cj, pj)]
    torch.cuda.synchronize()
    return tuple(t.data_ptr() for t in keep), keep


@pytest.fixture(scope="module")
def cell_items(oracle):
    return _Dev(_sidecar(oracle, S.MODE_REFERENCE))


def test_a_handle_of_the_other_kind_is_refused(K, gpu_setup, blob_ptrs, cell_items):
    l = K.lib()
    bv, cv = K.Verifier(gpu_setup, N_BLOBS), K.CellVerifier(gpu_setup, 64)
    try:
        with _mode(K, gpu_setup, S.MODE_REFERENCE):
            # the blob verifier's handle at the cells' entry points
            res = K.CellVerifyResult()
            assert l.lwkzg_cell_verifier_pending(bv.h) == -1 and l.lwkzg_cell_verifier_wait(bv.h) == K.C_KZG_BADARGS
            assert l.lwkzg_cell_verifier_enqueue(bv.h, C.byref(res), *cell_items.ptrs(), cell_items.n, None) == K.C_KZG_BADARGS
            assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, NONE_BAD)
            l.lwkzg_cell_verifier_free(bv.h)
            # the cell verifier's handle at the blobs' entry points
            res = K.VerifyResult()
            assert l.lwkzg_verifier_pending(cv.h) == -1 and l.lwkzg_verifier_wait(cv.h) == K.C_KZG_BADARGS
            assert l.lwkzg_verifier_enqueue(cv.h, C.byref(res), *blob_ptrs[0], N_BLOBS, None) == K.C_KZG_BADARGS
            assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, NONE_BAD)
            l.lwkzg_verifier_free(cv.h)
            # nothing was done to either: both are live, idle, and verify an honest batch
            assert (bv.pending(), cv.pending()) == (0, 0)
            rb, rc = bv.enqueue(*blob_ptrs[0], N_BLOBS), cv.enqueue(*cell_items.ptrs(), cell_items.n)
            bv.wait()
            cv.wait()
            assert (rb.state, rb.rc, rb.ok, rb.first_bad) == (1, 0, 1, NONE_BAD)
            assert (rc.state, rc.rc, rc.ok, rc.first_bad) == (1, 0, 1, NONE_BAD)
    finally:
        bv.free()
        cv.free()
    assert (bv.pending(), cv.pending()) == (-1, -1)


def test_one_setup_freed_under_a_call_in_flight_of_each_kind(K, blob_ptrs, cell_items):
    """free_trusted_setup waits for the calls in flight of both verifiers; both then refuse, and are still freed cleanly"""
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    ts.set_mode(K.MODE_REFERENCE)
    bv, cv = K.Verifier(ts, N_BLOBS), K.CellVerifier(ts, 64)
    rb, rc = bv.enqueue(*blob_ptrs[0], N_BLOBS), cv.enqueue(*cell_items.ptrs(), cell_items.n)
    ts.free()
    assert (rb.state, rb.rc, rb.ok) == (1, 0, 1) and (rc.state, rc.rc, rc.ok) == (1, 0, 1)
    for v, args in ((bv, blob_ptrs[0] + (N_BLOBS,)), (cv, cell_items.ptrs() + (cell_items.n,))):
        with pytest.raises(K.KzgError) as e:
            v.enqueue(*args)
        assert e.value.rc == K.C_KZG_BADARGS and (e.value.result.state, e.value.result.rc) == (1, K.C_KZG_BADARGS)
        v.free()
        assert v.pending() == -1
