"""CPU: what the batch verification of openings has that needs no GPU -- the five symbols in the header, the
export list and the binding; the host half of a call (the challenge over records built from openings, [sum r^i y_i]G, the pairing,
the partial) through lwkzg_verifier_host_steps, with the three sums from the oracle's MSM and the truth from its known-tau check;
and the argument errors that are decided before any device work."""
import ctypes as C
import hashlib
import os
import re
import struct

import pytest

import blobs as B
from conftest import R, ROOT, TAU

NEW_SYMBOLS = ["lwkzg_verify_kzg_proof_batch", "lwkzg_verify_kzg_proof_batch_device", "lwkzg_verify_kzg_proof_batch_partial",
               "lwkzg_verifier_enqueue_openings", "lwkzg_verify_kzg_proof_each_device"]
NONE_BAD = 0xffffffff


def test_the_declarations_are_exported_and_bound(K):
    from lambdaworks_kzg_amd import capi
    header = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    l = K.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bC_KZG_RET %s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(l, name), name
        assert getattr(l, name).argtypes is not None, name
    for fn in ("verify_kzg_proof_batch", "verify_kzg_proof_batch_device", "verify_kzg_proof_batch_partial", "verify_kzg_proof_each_device"):
        assert callable(getattr(K, fn)) and getattr(K, fn) is getattr(capi, fn), fn
    assert callable(K.Verifier.enqueue_openings)
    src = open(os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc", "Makefile")).read()
    assert "verify_openings.hip" in src


def _hand_built_settings(capi, oracle, oracle_setup):
    def blst_fp(be48):
        return struct.pack("<6Q", *[int.from_bytes(be48[8 * k:8 * k + 8], "big") for k in range(6)])

    g2 = b""
    for k in (1, TAU):
        xy = oracle.g2_generator_mul(k)
        g2 += b"".join(blst_fp(xy[48 * j:48 * j + 48]) for j in range(4)) + blst_fp((1).to_bytes(48, "big")) + blst_fp(bytes(48))
    g1 = oracle_setup.g1_blst()[:144]
    keep = (C.create_string_buffer(g1, len(g1)), C.create_string_buffer(g2, len(g2)))
    s = capi.KZGSettings()
    s.fs, s.g1_values, s.g2_values = None, C.addressof(keep[0]), C.addressof(keep[1])
    return s, keep


@pytest.mark.parametrize("mode", [0, 1])
def test_host_half_on_records_built_from_openings(K, oracle, oracle_setup, mode):
    """n = 4 openings at points of the test's choosing (no blob challenge anywhere): the records and the three sums from the oracle,
    the two host steps from the library. The verdict is the conjunction of the oracle's known-tau checks: honest, one y altered, and
    y + 1 / y - 1 on the same opening, which only the weights r^i tell apart from an honest pair."""
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle, oracle_setup)
    order = "little" if mode else "big"
    items = []
    for i in range(4):
        blob = B.synthetic_blob(66000 + (i & 1), big_endian=not mode)   # two blobs, two points each
        rc, cm = oracle.blob_to_kzg_commitment(blob, oracle_setup, mode)
        assert rc == 0
        z = (0x1234567 * (i + 3) * 0x89abcdef % R).to_bytes(32, order)
        rc, pi, y = oracle.compute_kzg_proof(blob, z, oracle_setup, mode)
        assert rc == 0
        items.append((cm, z, y, pi))

    def be(x):
        return int(x).to_bytes(32, "big")

    def shift(item, d):
        cm, z, y, pi = item
        return (cm, z, ((int.from_bytes(y, order) + d) % R).to_bytes(32, order), pi)

    def host_steps(items):
        n = len(items)
        records = b"".join(b"".join(t) for t in items)
        r = int.from_bytes(hashlib.sha256(b"RCKZGBATCH___V1_" + struct.pack("<QQ", 4096, n) + records).digest(), order) % R
        pw = [pow(r, i, R) for i in range(n)]
        zs, ys = [int.from_bytes(t[1], order) for t in items], [int.from_bytes(t[2], order) for t in items]
        pts_p, pts_c = [oracle.g1_decompress(t[3]) for t in items], [oracle.g1_decompress(t[0]) for t in items]
        assert all(p is not None and not p[1] for p in pts_p + pts_c)
        sums97 = b""
        for pts, scalars in ((pts_p, pw), (pts_p, [a * b % R for a, b in zip(pw, zs)]), (pts_c, pw)):
            got = oracle.g1_decompress(oracle.msm_affine(b"".join(xy for xy, _ in pts), b"".join(be(x) for x in scalars)))
            sums97 += (b"\x01" + bytes(96)) if got[1] else (b"\x00" + got[0])
        ysum = sum(a * b for a, b in zip(pw, ys)) % R
        res = capi.verifier_host_steps(records, n, NONE_BAD, sums97, be(ysum), C.byref(s), mode)
        assert (res.state, res.rc, res.first_bad) == (1, 0, NONE_BAD)
        assert bytes(res.r) == be(r) == K.batch_challenge_host(records, n, mode)
        assert bytes(res.partial)[:291] == sums97 and bytes(res.partial)[291:323] == be(ysum)
        truth = []
        for t in items:
            rc, ok = oracle.verify_kzg_proof_known_tau(*t, TAU, mode)
            assert rc == 0
            truth.append(ok)
        assert bool(res.ok) == all(truth), truth
        return bool(res.ok)

    assert host_steps(items) is True
    assert host_steps(items[:1]) is True
    assert host_steps([items[0], shift(items[1], 1), items[2], items[3]]) is False
    assert host_steps([items[0], shift(items[1], 1), shift(items[1], -1), items[3]]) is False
    assert host_steps([items[0], shift(items[1], -1), shift(items[1], 1), items[3]]) is False
    assert host_steps([items[0], items[1], items[1], items[3]]) is True


def test_argument_errors_decided_before_any_device_work(K, oracle, oracle_setup):
    """on settings put together by hand, which no context stands behind: every answer here comes from the entry points' own checks"""
    from lambdaworks_kzg_amd import capi
    l = K.lib()
    s, keep = _hand_built_settings(capi, oracle, oracle_setup)
    ok = C.c_bool(True)
    c48, s32 = bytes(48), bytes(32)
    try:
        for mode, code, empty in ((K.MODE_REFERENCE, K.C_KZG_ERROR, False), (K.MODE_CKZG, K.C_KZG_BADARGS, True), (K.MODE_ETH, K.C_KZG_BADARGS, True)):
            K.set_mode(mode)
            assert l.lwkzg_verify_kzg_proof_batch(None, c48, s32, s32, c48, 1, C.byref(s)) == K.C_KZG_BADARGS
            assert l.lwkzg_verify_kzg_proof_batch_device(None, 0x1000, 0x2000, 0x3000, 0x4000, 1, C.byref(s), None) == K.C_KZG_BADARGS
            for device in (False, True):
                ok.value = not empty
                if device:
                    assert l.lwkzg_verify_kzg_proof_batch_device(C.byref(ok), None, None, None, None, 0, C.byref(s), None) == 0
                else:
                    assert l.lwkzg_verify_kzg_proof_batch(C.byref(ok), None, None, None, None, 0, C.byref(s)) == 0
                assert ok.value is empty
            for hole in range(4):
                args = [c48, s32, s32, c48]
                args[hole] = None
                ok.value = True
                assert l.lwkzg_verify_kzg_proof_batch(C.byref(ok), *args, 2, C.byref(s)) == code
                assert ok.value is False
                ptrs = [0x1000, 0x2000, 0x3000, 0x4000]
                ptrs[hole] = None
                assert l.lwkzg_verify_kzg_proof_batch_device(C.byref(ok), *ptrs, 2, C.byref(s), None) == code
                ptrs = [0x1000, 0x2000, 0x3000, 0x4000]
                ptrs[hole] += 4
                assert l.lwkzg_verify_kzg_proof_batch_device(C.byref(ok), *ptrs, 2, C.byref(s), None) == K.C_KZG_BADARGS
            assert l.lwkzg_verify_kzg_proof_batch(C.byref(ok), c48, s32, s32, c48, 1, None) == code
            r, partial = C.create_string_buffer(32), C.create_string_buffer(328)
            assert l.lwkzg_verify_kzg_proof_batch_partial(None, partial, c48, s32, s32, c48, 1, C.byref(s)) == K.C_KZG_BADARGS
            assert l.lwkzg_verify_kzg_proof_batch_partial(r, None, c48, s32, s32, c48, 1, C.byref(s)) == K.C_KZG_BADARGS
            assert l.lwkzg_verify_kzg_proof_batch_partial(r, partial, None, s32, s32, c48, 1, C.byref(s)) == code
            assert l.lwkzg_verify_kzg_proof_batch_partial(r, partial, None, None, None, None, 0, C.byref(s)) == 0
            assert r.raw == bytes(32) and partial.raw == bytes(328)
    finally:
        K.set_mode(K.MODE_REFERENCE)
    # the verifier's entry point: a NULL handle is refused with the result complete, a NULL result with nothing to complete
    res = K.VerifyResult()
    C.memset(C.byref(res), 0xa5, C.sizeof(res))
    assert l.lwkzg_verifier_enqueue_openings(None, C.byref(res), None, None, None, None, 5, None) == K.C_KZG_BADARGS
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, NONE_BAD)
    assert bytes(res)[16:] == bytes(C.sizeof(res) - 16)
    assert l.lwkzg_verifier_enqueue_openings(None, None, None, None, None, None, 5, None) == K.C_KZG_BADARGS
    ok8, rc32 = (C.c_uint8 * 1)(), (C.c_int32 * 1)()
    assert l.lwkzg_verify_kzg_proof_each_device(None, rc32, None, None, None, None, 1, C.byref(s), None) == K.C_KZG_BADARGS
    assert l.lwkzg_verify_kzg_proof_each_device(ok8, rc32, None, None, None, None, 0, C.byref(s), None) == 0
    assert l.lwkzg_verify_kzg_proof_each_device(ok8, rc32, 0x1000, None, 0x3000, 0x4000, 1, C.byref(s), None) == K.C_KZG_BADARGS
