"""CPU: the parts of the asynchronous batch verifier (lwkzg_verifier_*) that need no GPU. The job slots and
their hand-over (lambdaworks_kzg_amd/csrc/verifier_ring.h) under -fsanitize=thread with a thread in the role of the runtime's
callback thread; the two host steps of an enqueue (the batch challenge of /root/reference/src/utils.rs:166-206, then
[sum r^i y_i]G, the pairing and the partial sums of /root/reference/src/lib.rs:679-691) through the host-only hook on a KZGSettings put
together by hand; the arithmetic of k_verify_ysum compiled for the host against the plain field; and the new symbols in the header,
the export list and the binding."""
import ctypes as C
import hashlib
import os
import re
import struct
import subprocess

import pytest

import blobs as B
from conftest import R, ROOT

NEW_SYMBOLS = ["lwkzg_verifier_new", "lwkzg_verifier_enqueue", "lwkzg_verifier_wait", "lwkzg_verifier_host_steps"]
NONE_BAD = 0xffffffff


def test_verifier_ring_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "verifier_ring_tsan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I", os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "verifier_ring_tsan.cpp"), "-o", exe])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    for producers, calls in ((6, 300), (16, 60)):
        out = subprocess.run([exe, str(producers), str(calls)], env=env, capture_output=True, timeout=600)
        text = out.stdout.decode() + out.stderr.decode()
        assert out.returncode == 0, text[-3000:]
        assert "ThreadSanitizer" not in text and "%d jobs, 0 check failures" % (producers * calls) in text, text[-3000:]


def test_ysum_arithmetic_on_the_host(tmp_path):
    """the arithmetic of k_verify_ysum (csrc/verify_ysum.cuh: a lane's share, the tree's addition, the canonical bytes), compiled for
    the host and run lane after lane against sum r^i y_i on the plain field: tests/verify_ysum_check.hip"""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "verify_ysum_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-I", os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "verify_ysum_check.hip"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("ok: 128 cases"), out


def _hand_built_settings(capi, oracle, oracle_setup):
    def blst_fp(be48):
        return struct.pack("<6Q", *[int.from_bytes(be48[8 * k:8 * k + 8], "big") for k in range(6)])

    g2 = b""
    for k in (1, 1337):
        xy = oracle.g2_generator_mul(k)
        g2 += b"".join(blst_fp(xy[48 * j:48 * j + 48]) for j in range(4)) + blst_fp((1).to_bytes(48, "big")) + blst_fp(bytes(48))
    g1 = oracle_setup.g1_blst()[:144]
    keep = (C.create_string_buffer(g1, len(g1)), C.create_string_buffer(g2, len(g2)))
    s = capi.KZGSettings()
    s.fs, s.g1_values, s.g2_values = None, C.addressof(keep[0]), C.addressof(keep[1])
    return s, keep


@pytest.mark.parametrize("mode", [0, 1])
def test_host_steps_without_a_gpu(K, oracle, oracle_setup, mode):
    """n = 3: the records and the three sums from the CPU reference implementation, the two host steps from the library. Honest ->
    ok, and r is SHA-256 of the transcript reduced mod r; one y altered -> not ok; a rejected index -> the mode's code and nothing
    else is read."""
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle, oracle_setup)
    n, order = 3, "little" if mode else "big"
    items = []
    for i in range(n):
        blob = B.synthetic_blob(64000 + i, big_endian=not mode)
        rc, cm = oracle.blob_to_kzg_commitment(blob, oracle_setup, mode)
        assert rc == 0
        rc, z = oracle.compute_challenge(blob, cm, mode)
        assert rc == 0
        rc, pi, y = oracle.compute_kzg_proof(blob, z, oracle_setup, mode)
        assert rc == 0 and (0, pi) == oracle.compute_blob_kzg_proof(blob, cm, oracle_setup, mode)
        items.append((cm, z, y, pi))

    def be(x):
        return int(x).to_bytes(32, "big")

    def blocks(items):
        records = b"".join(cm + z + y + pi for cm, z, y, pi in items)
        digest = hashlib.sha256(b"RCKZGBATCH___V1_" + struct.pack("<QQ", 4096, n) + records).digest()
        r = int.from_bytes(digest, order) % R
        sums, ysum, rp = [(bytes(96), True)] * 3, 0, 1
        for cm, z, y, pi in items:
            zi, yi = int.from_bytes(z, order), int.from_bytes(y, order)
            rz = int.from_bytes(oracle.fr_mul(be(rp), be(zi)), "big")
            ysum = (ysum + int.from_bytes(oracle.fr_mul(be(rp), be(yi)), "big")) % R
            (pxy, pinf), (cxy, cinf) = oracle.g1_decompress(pi), oracle.g1_decompress(cm)
            terms = ((pxy, pinf, rp), (pxy, pinf, rz), (cxy, cinf, rp))
            for k, (xy, inf, sc) in enumerate(terms):
                t = (bytes(96), True) if inf else oracle.g1_mul_affine(xy, sc)
                sums[k] = oracle.g1_add_affine(sums[k][0], sums[k][1], t[0], t[1])
            rp = rp * r % R
        sums97 = b"".join((b"\x01" + bytes(96)) if inf else (b"\x00" + xy) for xy, inf in sums)
        return records, r, sums97, ysum

    records, r, sums97, ysum = blocks(items)
    res = capi.verifier_host_steps(records, n, NONE_BAD, sums97, be(ysum), C.byref(s), mode)
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 1, NONE_BAD)
    assert bytes(res.r) == be(r)
    assert bytes(res.partial)[:291] == sums97 and bytes(res.partial)[291:323] == be(ysum)
    # one y altered: another transcript, another r, and sums that no longer balance
    cm, z, y, pi = items[1]
    wrong = list(items)
    wrong[1] = (cm, z, ((int.from_bytes(y, order) + 1) % R).to_bytes(32, order), pi)
    records2, r2, sums2, ysum2 = blocks(wrong)
    res = capi.verifier_host_steps(records2, n, NONE_BAD, sums2, be(ysum2), C.byref(s), mode)
    assert (res.state, res.rc, res.ok) == (1, 0, 0) and bytes(res.r) == be(r2) and r2 != r
    # a rejected input: the mode's code, the blocks are not read (none are given)
    res = capi.verifier_host_steps(None, n, 1, None, None, C.byref(s), mode)
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS if mode else K.C_KZG_ERROR, 0, 1)
    assert bytes(res.r) == bytes(32) and bytes(res.partial) == bytes(328)


def test_new_symbols_are_declared_exported_and_bound(K):
    from lambdaworks_kzg_amd import capi
    header = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    l = K.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bC_KZG_RET %s\(" % name, header), name
    assert re.search(r"\bint\s+lwkzg_verifier_pending\(", header) and re.search(r"\bvoid\s+lwkzg_verifier_free\(", header)
    for name in NEW_SYMBOLS + ["lwkzg_verifier_pending", "lwkzg_verifier_free"]:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(l, name), name
    assert "#define LWKZG_VERIFIER_DEPTH %d" % K.VERIFIER_DEPTH in header
    assert C.sizeof(K.VerifyResult) == 16 + 32 + 328 and K.VerifyResult.partial.offset == 48
    for method in ("enqueue", "pending", "wait", "free"):
        assert hasattr(K.Verifier, method), method
    # no GPU is needed to be refused
    res = K.VerifyResult()
    assert l.lwkzg_verifier_enqueue(None, C.byref(res), None, None, None, 0, None) == K.C_KZG_BADARGS
    assert (res.state, res.rc) == (1, K.C_KZG_BADARGS)
    assert l.lwkzg_verifier_pending(None) == -1 and l.lwkzg_verifier_wait(None) == K.C_KZG_BADARGS
    l.lwkzg_verifier_free(None)


def test_a_null_handle_is_answered_alike_by_both_kinds(K):
    """the entry points the two kinds share (csrc/async_verifier.h): pending -1, wait BADARGS, enqueue BADARGS with the result
    complete -- zeroed but for state, rc and first_bad --, and BADARGS with nothing to complete when the result is NULL too"""
    l = K.lib()
    for prefix, result, pointers in (("lwkzg_verifier_", K.VerifyResult, 3), ("lwkzg_cell_verifier_", K.CellVerifyResult, 4)):
        fn = lambda name: getattr(l, prefix + name)
        assert fn("pending")(None) == -1 and fn("wait")(None) == K.C_KZG_BADARGS
        res = result()
        C.memset(C.byref(res), 0xa5, C.sizeof(res))
        assert fn("enqueue")(None, C.byref(res), *([None] * pointers), 5, None) == K.C_KZG_BADARGS
        assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, NONE_BAD)
        assert bytes(res)[16:] == bytes(C.sizeof(res) - 16)
        assert fn("enqueue")(None, None, *([None] * pointers), 5, None) == K.C_KZG_BADARGS
        fn("free")(None)
