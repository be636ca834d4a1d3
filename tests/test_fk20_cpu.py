"""CPU: the FK20 cell proof engine (lwkzg_set_cell_proof_engine, lwkzg_cell_proof_engine, lwkzg_fk20_*) as far as it goes without a
GPU: its formulas (tests/fk20_spec.py) held against cells_spec.quotient on a toy linear group with unstructured points; the argument
checks, which are decided before any device work; and the host+device pieces of its kernels (csrc/fk20.cuh) compiled for the host and
held against g1.cuh's plain double-and-add (tools/fk20_check.hip), once plain and once under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import cells_spec as S
import fk20_spec as F
from conftest import R, ROOT, TAU


def _blobs():
    rnd = random.Random(2020)
    return {
        "random": [rnd.randrange(R) for _ in range(4096)],
        "zero": [0] * 4096,
        "constant": [12345] + [0] * 4095,
        "degree_below_64": [rnd.randrange(R) for _ in range(64)] + [0] * 4032,
        "x64": [0] * 64 + [1] + [0] * 4031,
        "all_r_minus_1": [R - 1] * 4096,
        "edge": F.edge_polynomial(TAU),
    }


@pytest.fixture(scope="module")
def toy():
    """unstructured "points" of the toy group and the bases over them"""
    rnd = random.Random(7594)
    G = [rnd.randrange(1, R) for _ in range(4096)]
    return G, F.bases(G)


@pytest.mark.parametrize("name", list(_blobs()))
def test_formulas_against_the_quotients(toy, name):
    G, yhat = toy
    p = _blobs()[name]
    want = F.proofs_by_quotients(p, G)
    for k in (0, 1, 77, 127):   # the definitions first: proof_k = sum_u c_k^u h_u
        h = F.h_direct(p, G)
        assert sum(pow(S.c_of_cell(k), u, R) * h[u] for u in range(64)) % R == want[k], k
    e = F.e_points(p, yhat)
    h, discarded = F.h_from_e(e)
    assert h == F.h_direct(p, G) and h[63] == 0
    assert F.proofs_from_h(h) == want
    if name == "random":
        assert any(discarded)   # entries 64 .. 127 are not zero by themselves: they are replaced


def test_the_edge_blob_on_a_powers_of_tau_setup():
    G = [pow(TAU, t, R) for t in range(4096)]   # the toy group's generator is 1
    p = F.edge_polynomial(TAU)
    h = F.h_direct(p, G)
    assert h[0] == 1 and h[32] == 1 and not any(h[u] for u in range(64) if u not in (0, 32))
    proofs = F.proofs(p, G)
    assert proofs == F.proofs_by_quotients(p, G)
    assert proofs == [(1 + pow(F.W, 32 * S.rev(k, 7), R)) % R for k in range(128)]
    assert proofs.count(2) == 32 and proofs.count(0) == 32


def test_argument_checks_are_decided_before_any_device_work(K):
    l = K.lib()
    s = K.KZGSettings()           # hand-made: no context behind it
    for engine, bits in ((0, 0), (1, 0), (7, 0), (1, 99)):
        assert l.lwkzg_set_cell_proof_engine(None, engine, bits, 0) == K.C_KZG_BADARGS
    assert l.lwkzg_set_cell_proof_engine(C.byref(s), 7, 0, 0) == K.C_KZG_BADARGS
    assert l.lwkzg_set_cell_proof_engine(C.byref(s), -1, 0, 0) == K.C_KZG_BADARGS
    for bits in (99, 5, 10, 3, -8):
        assert l.lwkzg_set_cell_proof_engine(C.byref(s), K.CELL_PROOFS_FK20, bits, 0) == K.C_KZG_BADARGS, bits
    assert l.lwkzg_set_cell_proof_engine(C.byref(s), K.CELL_PROOFS_MSM, 99, 0) == K.C_KZG_BADARGS
    # good arguments on settings without a context: refused as every other call refuses them
    assert l.lwkzg_set_cell_proof_engine(C.byref(s), K.CELL_PROOFS_FK20, 8, 1) == K.C_KZG_ERROR
    assert l.lwkzg_cell_proof_engine(None) == -1 and l.lwkzg_cell_proof_engine(C.byref(s)) == -1
    assert l.lwkzg_fk20_table_bytes(None) == 0 and l.lwkzg_fk20_table_bytes(C.byref(s)) == 0
    assert l.lwkzg_fk20_chunk_blobs() == K.fk20_chunk_blobs() > 8
    out = C.create_string_buffer(b"\x55" * 97, 97)
    blob = bytes(K.BYTES_PER_BLOB)
    assert l.lwkzg_fk20_points(out, 1, blob, None) == K.C_KZG_BADARGS
    assert l.lwkzg_fk20_points(None, 1, blob, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_fk20_points(out, 3, blob, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_fk20_points(out, 2, None, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_fk20_points(out, 1, blob, C.byref(s)) == K.C_KZG_ERROR
    assert out.raw == b"\x55" * 97


def test_python_wrappers_are_exported(K):
    for name in ("set_cell_proof_engine", "cell_proof_engine", "fk20_table_bytes", "fk20_points"):
        assert callable(getattr(K.TrustedSetup, name)), name
    assert callable(K.fk20_chunk_blobs) and K.capi.fk20_chunk_blobs is K.fk20_chunk_blobs
    assert (K.CELL_PROOFS_MSM, K.CELL_PROOFS_FK20) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    assert "#define LWKZG_CELL_PROOFS_MSM  0" in hdr and "#define LWKZG_CELL_PROOFS_FK20 1" in hdr
    assert "#define LWKZG_FK20_DEFAULT_MIN_BLOBS %d" % K.capi.FK20_DEFAULT_MIN_BLOBS in hdr


@pytest.mark.parametrize("sanitized", [False, True])
def test_fk20_pieces_host_crosscheck(tmp_path, sanitized):
    """csrc/fk20.cuh compiled for the host: the fixed-root product of an XYZZ point for all 256 recoded roots (and P = O), the window
    digits of every supported width (0, 1, r - 1, carries into the top window), and both 128-point G1 transforms run position by
    position through the kernel's own functions against the O(n^2) sums (tools/fk20_check.hip). The second run is the same program
    under -fsanitize=address,undefined, a process of its own."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "fk20_check")
    extra = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else []
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only"] + extra +
                          ["-I", os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"), os.path.join(ROOT, "tools", "fk20_check.hip"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("ok:"), out
