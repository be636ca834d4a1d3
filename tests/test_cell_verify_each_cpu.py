"""CPU: per-item EIP-7594 cell proof verification (lwkzg_verify_cell_kzg_proof_each, _device, lwkzg_cell_verify_each_points) as far as
it goes without a GPU: the argument checks, which are decided before any device work, and the per-lane arithmetic of its kernels
(csrc/cell_each.cuh) compiled for the host and held against the plain double-and-add (tools/cell_each_check.hip)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_argument_checks_are_decided_before_any_device_work(K):
    l = K.lib()
    s = K.KZGSettings()           # hand-made: no context behind it
    ok = (C.c_uint8 * 2)(7, 7)
    rc = (C.c_int32 * 2)(-5, -5)
    idx = (C.c_uint64 * 2)(0, 1)
    comm, cells, proofs = bytes(96), bytes(4096), bytes(96)
    pts = C.create_string_buffer(b"\x55" * (2 * K.capi.CELL_EACH_POINT_BYTES), 2 * K.capi.CELL_EACH_POINT_BYTES)
    dev = C.c_void_p(4096)        # never dereferenced: every call below is refused, or has nothing to do, before it is looked at

    # n == 0: C_KZG_OK, nothing written -- with arguments and without
    assert l.lwkzg_verify_cell_kzg_proof_each(ok, rc, comm, idx, cells, proofs, 0, C.byref(s)) == K.C_KZG_OK
    assert l.lwkzg_verify_cell_kzg_proof_each(None, None, None, None, None, None, 0, C.byref(s)) == K.C_KZG_OK
    assert l.lwkzg_verify_cell_kzg_proof_each_device(ok, rc, dev, dev, dev, dev, 0, C.byref(s), None) == K.C_KZG_OK
    assert l.lwkzg_verify_cell_kzg_proof_each_device(None, None, None, None, None, None, 0, C.byref(s), None) == K.C_KZG_OK
    assert l.lwkzg_cell_verify_each_points(pts, comm, idx, cells, proofs, 0, C.byref(s)) == K.C_KZG_OK
    assert l.lwkzg_cell_verify_each_points(None, None, None, None, None, 0, C.byref(s)) == K.C_KZG_OK
    assert list(ok) == [7, 7] and list(rc) == [-5, -5] and pts.raw == b"\x55" * (2 * K.capi.CELL_EACH_POINT_BYTES)

    # s NULL: C_KZG_BADARGS, whatever n
    for n in (0, 2):
        assert l.lwkzg_verify_cell_kzg_proof_each(ok, rc, comm, idx, cells, proofs, n, None) == K.C_KZG_BADARGS
        assert l.lwkzg_verify_cell_kzg_proof_each_device(ok, rc, dev, dev, dev, dev, n, None, None) == K.C_KZG_BADARGS
        assert l.lwkzg_cell_verify_each_points(pts, comm, idx, cells, proofs, n, None) == K.C_KZG_BADARGS

    # any NULL pointer with n > 0: C_KZG_BADARGS
    host_args = [ok, rc, comm, idx, cells, proofs]
    for hole in range(6):
        a = list(host_args)
        a[hole] = None
        assert l.lwkzg_verify_cell_kzg_proof_each(*a, 2, C.byref(s)) == K.C_KZG_BADARGS, hole
    dev_args = [ok, rc, dev, dev, dev, dev]
    for hole in range(6):
        a = list(dev_args)
        a[hole] = None
        assert l.lwkzg_verify_cell_kzg_proof_each_device(*a, 2, C.byref(s), None) == K.C_KZG_BADARGS, hole
    point_args = [pts, comm, idx, cells, proofs]
    for hole in range(5):
        a = list(point_args)
        a[hole] = None
        assert l.lwkzg_cell_verify_each_points(*a, 2, C.byref(s)) == K.C_KZG_BADARGS, hole
    assert list(ok) == [7, 7] and list(rc) == [-5, -5] and pts.raw == b"\x55" * (2 * K.capi.CELL_EACH_POINT_BYTES)

    # what the batch call refuses as a whole is refused the same way: settings without a context
    batch_ok = C.c_bool(True)
    want = l.lwkzg_verify_cell_kzg_proof_batch(C.byref(batch_ok), comm, idx, cells, proofs, 2, C.byref(s))
    assert want == K.C_KZG_ERROR
    assert l.lwkzg_verify_cell_kzg_proof_each(ok, rc, comm, idx, cells, proofs, 2, C.byref(s)) == want
    assert l.lwkzg_cell_verify_each_points(pts, comm, idx, cells, proofs, 2, C.byref(s)) == want


def test_python_wrappers_are_exported(K):
    for name in ("verify_cell_kzg_proof_each", "verify_cell_kzg_proof_each_device", "cell_verify_each_points"):
        assert callable(getattr(K, name)) and getattr(K.capi, name) is getattr(K, name)
    assert K.capi.CELL_EACH_POINT_BYTES == 97
    hdr = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    assert "#define LWKZG_CELL_EACH_POINT_BYTES 97" in hdr


def test_two_base_scalar_product_host_crosscheck(tmp_path):
    """csrc/cell_each.cuh compiled for the host: [k]Q over the endomorphism split (the per-lane product of k_celleach_commit and
    k_celleach_combine) against g1.cuh's plain double-and-add on 0, 1, z^2 - 1, z^2, z^2 + 1, 2^128 - 1, 2^128, r - 1, every c_k and
    random scalars, for the generator and a second point; and the scalar conversions (tools/cell_each_check.hip)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "cell_each_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-I", os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"),
                           os.path.join(ROOT, "tools", "cell_each_check.hip"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("ok:"), out
