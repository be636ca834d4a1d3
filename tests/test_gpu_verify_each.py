"""GPU: per-item verification (lwkzg_verify_blob_kzg_proof_each, its _device form, lwkzg_verify_kzg_proof_each). For every item the
(rc, ok) of the call equals, byte for byte, what the single verify_blob_kzg_proof / verify_kzg_proof answers on that item
(the reference's src/lib.rs:456-505, 407-453), in both modes: honest items, swapped proofs / commitments / blobs, invalid encodings,
a non-canonical blob element, a non-canonical infinity encoding of C, the zero blob, pi = O with C != O. Independent truth from the
oracle's known-tau check (no pairing code), agreement with the batch verification, a second setup in the same process, both MSM engines,
inputs produced on the caller's stream, the empty call."""
import ctypes as C
import os
import random

import pytest

import blobs as B
from conftest import GOLDEN, R, TAU, hx

pytestmark = pytest.mark.gpu

INF = bytes([0xc0]) + bytes(47)


def _dev(torch, data):
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


def _single_blob(K, blob, c, p, ts):
    ok = C.c_bool(False)
    rc = K.lib().verify_blob_kzg_proof(C.byref(ok), blob, c, p, ts.ref())
    return rc, bool(ok.value)


def _single_opening(K, c, z, y, p, ts):
    ok = C.c_bool(False)
    rc = K.lib().verify_kzg_proof(C.byref(ok), c, z, y, p, ts.ref())
    return rc, bool(ok.value)


def _each_device(K, torch, blobs, comms, proofs, n, ts, stream=None):
    db, dc, dp = _dev(torch, blobs), _dev(torch, comms), _dev(torch, proofs)
    torch.cuda.synchronize()
    return K.verify_blob_kzg_proof_each_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, ts, stream)


def _honest(K, n, seed, le, ts):
    blobs = [B.synthetic_blob(seed + i, big_endian=not le) for i in range(n)]
    data = b"".join(blobs)
    cms = K.blob_to_kzg_commitment_batch(data, ts)
    prs = K.compute_blob_kzg_proof_batch(data, b"".join(cms), ts)
    return blobs, list(cms), list(prs)


def _mixed(K, n, seed, le, ts):
    """honest items with every kind of defect mixed in at random places (n >= 2: a swap needs a neighbour)"""
    rnd = random.Random(seed)
    blobs, cms, prs = _honest(K, n, seed, le, ts)
    zero_c = INF
    kinds = ["swap_proof", "swap_commitment", "swap_blob", "bad_c", "bad_pi", "elem", "inf_noncanon", "zero", "pi_inf"]
    places = list(range(n))
    rnd.shuffle(places)
    per = max(1, n // 24) if n >= 24 else 1
    k = 0
    for kind in kinds:
        for _ in range(per):
            if k >= len(places) or (n < 24 and k >= n - 1):
                break
            i = places[k]
            j = (i + 1) % n
            k += 1
            if kind == "swap_proof" and n > 1:
                prs[i] = prs[j]
            elif kind == "swap_commitment" and n > 1:
                cms[i] = cms[j]
            elif kind == "swap_blob" and n > 1:
                blobs[i] = blobs[j]
            elif kind == "bad_c":
                cms[i] = bytes([cms[i][0] & 0x7f]) + cms[i][1:]   # compression flag cleared: an invalid encoding
            elif kind == "bad_pi":
                prs[i] = bytes([0xa0]) + bytes(rnd.getrandbits(8) for _ in range(47))   # x of no curve point, or not canonical
            elif kind == "elem":
                b = bytearray(blobs[i])
                if le:
                    b[32 * 5 + 31] = 0xff                     # element 5 >= r
                else:
                    b[32 * 5] = 0xff
                blobs[i] = bytes(b)
            elif kind == "inf_noncanon":
                blobs[i] = bytes(B.BYTES_PER_BLOB)
                cms[i] = bytes([0xc0]) + bytes(46) + b"\x01"  # infinity flag with a stray bit
                prs[i] = INF
            elif kind == "zero":
                blobs[i], cms[i], prs[i] = bytes(B.BYTES_PER_BLOB), zero_c, INF
            elif kind == "pi_inf":
                prs[i] = INF
    return blobs, cms, prs


def _truth_blobs(K, blobs, cms, prs, ts):
    return [_single_blob(K, b, c, p, ts) for b, c, p in zip(blobs, cms, prs)]


@pytest.mark.parametrize("n", [1, 2, 64, 1025, 4096])
@pytest.mark.parametrize("mode", ["reference", "ckzg"])
def test_mixed_batches_match_the_single_calls(K, gpu_setup, n, mode):
    import torch
    le = mode == "ckzg"
    gpu_setup.set_mode(K.MODE_CKZG if le else K.MODE_REFERENCE)
    try:
        blobs, cms, prs = _mixed(K, n, 91000 + n + (7 if le else 0), le, gpu_setup)
        want = _truth_blobs(K, blobs, cms, prs, gpu_setup)
        got = K.verify_blob_kzg_proof_each(b"".join(blobs), b"".join(cms), b"".join(prs), gpu_setup)
        assert got == want
        got_dev = _each_device(K, torch, b"".join(blobs), b"".join(cms), b"".join(prs), n, gpu_setup)
        assert got_dev == want
        if n >= 64:   # every outcome is represented
            assert any(w == (0, True) for w in want) and any(w == (0, False) for w in want) and any(w[0] != 0 for w in want)
    finally:
        gpu_setup.set_mode(-1)


def test_independent_truth_known_tau(K, gpu_setup, oracle):
    """ok == the oracle's known-tau check (C - [y]G == [tau - z]pi: no pairing) on 96 validly encoded items"""
    n = 96
    blobs, cms, prs = _honest(K, n, 33000, False, gpu_setup)
    for i in range(0, n, 3):
        prs[i] = prs[(i + 1) % n]
    for i in range(1, n, 7):
        blobs[i] = blobs[(i + 2) % n]
    got = K.verify_blob_kzg_proof_each(b"".join(blobs), b"".join(cms), b"".join(prs), gpu_setup)
    zs = []
    for b, c in zip(blobs, cms):
        rc, z = oracle.compute_challenge(b, c, oracle.MODE_R)
        assert rc == 0
        zs.append(z)
    ys = [y for _, y in K.compute_kzg_proof_batch(b"".join(blobs), b"".join(zs), gpu_setup)]
    n_ok = 0
    for i in range(n):
        rc, ok = oracle.verify_kzg_proof_known_tau(cms[i], zs[i], ys[i], prs[i], TAU, oracle.MODE_R)
        assert rc == 0
        assert got[i] == (0, ok), i
        n_ok += ok
    assert 20 < n_ok < n - 20


def test_agreement_with_the_batch(K, gpu_setup):
    """an honest batch: all ok, batch true; k tampered items: batch false and exactly those k indices are 0"""
    import torch
    n = 300
    blobs, cms, prs = _honest(K, n, 47000, False, gpu_setup)
    assert K.verify_blob_kzg_proof_each(b"".join(blobs), b"".join(cms), b"".join(prs), gpu_setup) == [(0, True)] * n
    bad = sorted(random.Random(3).sample(range(n), 5))
    for i in bad:
        prs[i] = prs[(i + 1) % n]
    db, dc, dp = _dev(torch, b"".join(blobs)), _dev(torch, b"".join(cms)), _dev(torch, b"".join(prs))
    torch.cuda.synchronize()
    assert K.verify_blob_kzg_proof_batch_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, gpu_setup) is False
    got = K.verify_blob_kzg_proof_each_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, gpu_setup)
    assert [i for i, (rc, ok) in enumerate(got) if not ok] == bad
    assert all(rc == 0 for rc, _ in got)


@pytest.mark.parametrize("mode", ["reference", "ckzg"])
def test_openings_random(K, gpu_setup, oracle, mode):
    """honest openings, y + 1, z on the evaluation domain (c-kzg: the y the blob gives there), non-canonical z / y, invalid points:
    each item == the single verify_kzg_proof; in reference mode the verdicts also == the oracle's known-tau check"""
    le = mode == "ckzg"
    gpu_setup.set_mode(K.MODE_CKZG if le else K.MODE_REFERENCE)
    try:
        rnd = random.Random(808 + le)
        n = 80
        blobs, cms, _ = _honest(K, n, 61000 + 50 * le, le, gpu_setup)
        order = "little" if le else "big"
        zs = [rnd.randrange(R).to_bytes(32, order) for _ in range(n)]
        w = pow(7, (R - 1) // 4096, R)   # a 4096th root of unity: a z on the evaluation domain
        for i in range(0, n, 10):
            zs[i] = pow(w, rnd.randrange(4096), R).to_bytes(32, order)
        res = K.compute_kzg_proof_batch(b"".join(blobs), b"".join(zs), gpu_setup)
        prs, ys = [p for p, _ in res], [y for _, y in res]
        for i in range(1, n, 6):
            ys[i] = ((int.from_bytes(ys[i], order) + 1) % R).to_bytes(32, order)
        ys[5] = (R + 3).to_bytes(32, order)          # non-canonical y (reference mode: reduced)
        zs[7] = (2 ** 256 - 1).to_bytes(32, order)   # non-canonical z
        cms[9] = bytes([cms[9][0] & 0x7f]) + cms[9][1:]
        prs[11] = INF
        cms[13], prs[13], ys[13] = INF, INF, bytes(32)
        got = K.verify_kzg_proof_each(b"".join(cms), b"".join(zs), b"".join(ys), b"".join(prs), gpu_setup)
        want = [_single_opening(K, c, z, y, p, gpu_setup) for c, z, y, p in zip(cms, zs, ys, prs)]
        assert got == want
        assert sum(ok for _, ok in want) > 30 and sum(not ok for _, ok in want) > 10
        if not le:
            for i in range(n):
                if i in (5, 7, 9, 11, 13):
                    continue
                rc, ok = oracle.verify_kzg_proof_known_tau(cms[i], zs[i], ys[i], prs[i], TAU, oracle.MODE_R)
                assert rc == 0 and ok == got[i][1], i
    finally:
        gpu_setup.set_mode(-1)


def test_openings_ckzg_vectors(K, gpu_setup, vectors):
    """every case of the c-kzg verify_kzg_proof suite the fixed-size ABI can express, in one call: verdict or per-item C_KZG_BADARGS"""
    gpu_setup.set_mode(K.MODE_CKZG)
    try:
        items, want = [], []
        for c in vectors["suites"]["verify_kzg_proof"]:
            i = c["input"]
            cm, z, y, pr = hx(i["commitment"]), hx(i["z"]), hx(i["y"]), hx(i["proof"])
            if len(cm) != 48 or len(pr) != 48 or len(z) != 32 or len(y) != 32:
                continue
            items.append((cm, z, y, pr))
            want.append((K.C_KZG_BADARGS, False) if c["output"] is None else (0, c["output"]))
        assert len(items) >= 10
        got = K.verify_kzg_proof_each(*[b"".join(t[k] for t in items) for k in range(4)], gpu_setup)
        assert got == want
        assert got == [_single_opening(K, *t, gpu_setup) for t in items]
    finally:
        gpu_setup.set_mode(-1)


def test_second_setup_in_the_same_process(K, gpu_setup):
    """the tau' setup and the tau = 1337 one each verify with their own G2 points: honest items of one are rejected by the other"""
    ts2 = K.TrustedSetup.from_file(os.path.join(GOLDEN, "trusted_setup_tau2.txt"))
    try:
        n = 40
        b1, c1, p1 = _honest(K, n, 71000, False, gpu_setup)
        b2, c2, p2 = _honest(K, n, 72000, False, ts2)
        j = lambda x: b"".join(x)   # noqa: E731
        assert K.verify_blob_kzg_proof_each(j(b1), j(c1), j(p1), gpu_setup) == [(0, True)] * n
        assert K.verify_blob_kzg_proof_each(j(b2), j(c2), j(p2), ts2) == [(0, True)] * n
        assert K.verify_blob_kzg_proof_each(j(b1), j(c1), j(p1), ts2) == _truth_blobs(K, b1, c1, p1, ts2)
        assert not any(ok for _, ok in K.verify_blob_kzg_proof_each(j(b1), j(c1), j(p1), ts2))
        assert K.verify_blob_kzg_proof_each(j(b2), j(c2), j(p2), gpu_setup) == _truth_blobs(K, b2, c2, p2, gpu_setup)
    finally:
        ts2.free()


def test_engines_give_identical_verdicts(K, gpu_setup):
    """the default engine and the bucket engine (enable_direct_table(0))"""
    n = 130
    blobs, cms, prs = _mixed(K, n, 12345, False, gpu_setup)
    j = lambda x: b"".join(x)   # noqa: E731
    a = K.verify_blob_kzg_proof_each(j(blobs), j(cms), j(prs), gpu_setup)
    gpu_setup.enable_direct_table(0)
    try:
        b = K.verify_blob_kzg_proof_each(j(blobs), j(cms), j(prs), gpu_setup)
    finally:
        gpu_setup.enable_direct_table(gpu_setup.default_bits)
    assert a == b == _truth_blobs(K, blobs, cms, prs, gpu_setup)


def test_inputs_from_the_callers_stream(K, gpu_setup):
    """inputs copied on the caller's own stream (not synchronised by the caller) are waited for"""
    import torch
    n = 200
    blobs, cms, prs = _mixed(K, n, 999, False, gpu_setup)
    want = _truth_blobs(K, blobs, cms, prs, gpu_setup)
    hb, hc, hp = (torch.frombuffer(bytearray(b"".join(x)), dtype=torch.uint8).pin_memory() for x in (blobs, cms, prs))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        db, dc, dp = (torch.empty(t.numel(), dtype=torch.uint8, device="cuda") for t in (hb, hc, hp))
        torch.cuda._sleep(20_000_000)   # the copies land well after the call starts
        db.copy_(hb, non_blocking=True)
        dc.copy_(hc, non_blocking=True)
        dp.copy_(hp, non_blocking=True)
    got = K.verify_blob_kzg_proof_each_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, gpu_setup, s.cuda_stream)
    assert got == want


def test_empty_call_and_null_pointers(K, gpu_setup):
    for mode in (K.MODE_REFERENCE, K.MODE_CKZG):
        gpu_setup.set_mode(mode)
        try:
            assert K.verify_blob_kzg_proof_each(b"", b"", b"", gpu_setup) == []
            assert K.verify_blob_kzg_proof_each_device(None, None, None, 0, gpu_setup) == []
            assert K.verify_kzg_proof_each(b"", b"", b"", b"", gpu_setup) == []
        finally:
            gpu_setup.set_mode(-1)
    l = K.lib()
    ok, rc = (C.c_uint8 * 1)(), (C.c_int32 * 1)()
    assert l.lwkzg_verify_blob_kzg_proof_each(None, rc, b"", b"", b"", 0, gpu_setup.ref()) == K.C_KZG_BADARGS
    assert l.lwkzg_verify_blob_kzg_proof_each(ok, rc, None, None, None, 1, gpu_setup.ref()) == K.C_KZG_BADARGS
    assert l.lwkzg_verify_kzg_proof_each(ok, None, None, None, None, None, 0, gpu_setup.ref()) == K.C_KZG_BADARGS
