"""CPU: what the consensus-specs mode (LWKZG_MODE_ETH = 2) decides without a GPU -- the mode switch and its environment variable, the
two Fiat-Shamir transcripts against hashlib (tests/eth_spec.py), the cell batch's challenge, verify_kzg_proof on a KZGSettings put
together by hand (big-endian AND canonical z / y), and the verifier's host steps."""
import ctypes as C
import hashlib
import json
import os
import random
import struct
import subprocess
import sys

import blobs as B
import eth_spec as E
from conftest import R, ROOT

ETH = 2
NONE_BAD = 0xffffffff


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


def _opening(oracle, rnd, tau=1337):
    """a true opening over the tau = 1337 setup: C = [y + (tau - z) a]G, pi = [a]G"""
    z, y, a = rnd.randrange(R), rnd.randrange(R), rnd.randrange(1, R)
    return oracle.g1_generator_mul((y + (tau - z) * a) % R), z, y, oracle.g1_generator_mul(a)


def test_mode_switching(K):
    assert K.MODE_ETH == ETH
    start = K.get_mode()
    try:
        assert K.set_mode(ETH) == start
        assert K.get_mode() == ETH
        assert K.set_mode(7) == -1 and K.get_mode() == ETH     # an unknown mode leaves the mode alone
        assert K.set_mode(K.MODE_CKZG) == ETH
    finally:
        K.set_mode(start)
    rep = K.knob_report()
    assert rep["mode"] in (0, 1, 2)
    size = K.lib().lwkzg_knob_report(None, 0)
    buf = C.create_string_buffer(size)
    assert K.lib().lwkzg_knob_report(buf, size) == size
    assert json.loads(buf.value.decode())["mode"] == rep["mode"]


def test_environment_variable_selects_the_mode():
    code = "import lambdaworks_kzg_amd as K; print(K.get_mode(), K.knob_report()['mode'])"
    for value, want in (("eth", "2 2"), ("ckzg", "1 1"), ("reference", "0 0")):
        env = dict(os.environ, LWKZG_MODE=value)
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.split("\n")[0].strip() == want, (value, out.stdout)


def test_challenge_digests_host_mode(K):
    from lambdaworks_kzg_amd import capi
    rnd = random.Random(11)
    blobs = [B.synthetic_blob(71000 + i) for i in range(3)]
    comms = [bytes(rnd.getrandbits(8) for _ in range(48)) for _ in range(3)]   # (the digest does not look at what the 48 bytes are)
    got = capi.challenge_digests_host_mode(b"".join(blobs), b"".join(comms), ETH)
    for b, c, g in zip(blobs, comms, got):
        want = hashlib.sha256(b"FSBLOBVERIFY_V1_" + (4096).to_bytes(16, "big") + b + c).digest()
        assert g == want
        assert (int.from_bytes(g, "big") % R).to_bytes(32, "big") == E.challenge_eth(b, c)
    old = capi.challenge_digests_host(b"".join(blobs), b"".join(comms))
    assert old == [hashlib.sha256(b"FSBLOBVERIFY_V1_" + struct.pack("<QQ", 4096, 0) + b + c).digest() for b, c in zip(blobs, comms)]
    for mode in (0, 1):
        assert capi.challenge_digests_host_mode(b"".join(blobs), b"".join(comms), mode) == old
    assert got != old
    out = C.create_string_buffer(96)
    assert capi.lib().lwkzg_challenge_digests_host_mode(out, b"".join(blobs), b"".join(comms), 3, 7) == K.C_KZG_BADARGS


def test_batch_challenge_host(K):
    from lambdaworks_kzg_amd import capi
    rnd = random.Random(12)
    for n in (0, 1, 5):
        records = bytes(rnd.getrandbits(8) for _ in range(160 * n))
        got = capi.batch_challenge_host(records, n, ETH)
        digest = hashlib.sha256(b"RCKZGBATCH___V1_" + struct.pack(">QQ", 4096, n) + records).digest()
        assert got == (int.from_bytes(digest, "big") % R).to_bytes(32, "big") == E.batch_r_eth(records)
        assert got != capi.batch_challenge_host(records, n, 0)
        assert got != capi.batch_challenge_host(records, n, 1)


def test_cell_batch_challenge_host(K):
    """the cell batch's transcript is the library's own in every mode: eth mode reads the same digest as reference mode, big-endian"""
    from lambdaworks_kzg_amd import capi
    rnd = random.Random(13)
    cms = [bytes(rnd.getrandbits(8) for _ in range(48)) for _ in range(2)]
    items = [(cms[j], k, bytes(rnd.getrandbits(8) for _ in range(2048)), bytes(rnd.getrandbits(8) for _ in range(48)))
             for j, k in ((0, 0), (1, 127), (0, 64))]
    args = ([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], [it[3] for it in items])
    r_eth, r_ref, r_ckzg = (capi.cell_batch_challenge_host(*args, mode) for mode in (ETH, 0, 1))
    assert r_eth == r_ref and int.from_bytes(r_eth, "big") < R
    assert r_eth != r_ckzg


def test_verify_kzg_proof_on_hand_built_settings(K, oracle, oracle_setup):
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle, oracle_setup)
    rnd = random.Random(14)
    ok = C.c_bool(False)
    verify = capi.lib().verify_kzg_proof
    start = K.get_mode()
    try:
        K.set_mode(ETH)
        for _ in range(4):
            cm, z, y, pi = _opening(oracle, rnd)
            zb, yb = z.to_bytes(32, "big"), y.to_bytes(32, "big")
            assert verify(C.byref(ok), cm, zb, yb, pi, C.byref(s)) == 0 and ok.value is True
            assert verify(C.byref(ok), cm, zb, ((y + 1) % R).to_bytes(32, "big"), pi, C.byref(s)) == 0 and ok.value is False
            for bad in (R.to_bytes(32, "big"), b"\xff" * 32):      # r and 2^256 - 1: not canonical
                assert verify(C.byref(ok), cm, bad, yb, pi, C.byref(s)) == K.C_KZG_BADARGS
                assert verify(C.byref(ok), cm, zb, bad, pi, C.byref(s)) == K.C_KZG_BADARGS
            # the byte order is the mode's: the same opening given little-endian does not verify (or is not canonical)
            rc = verify(C.byref(ok), cm, zb[::-1], yb[::-1], pi, C.byref(s))
            assert rc == K.C_KZG_BADARGS or (rc == 0 and ok.value is False)
        # r - 1 is the largest canonical value
        cm, z, y, pi = _opening(oracle, rnd)
        y = R - 1
        cm = oracle.g1_generator_mul((y + (1337 - z) * 5) % R)
        assert verify(C.byref(ok), cm, z.to_bytes(32, "big"), y.to_bytes(32, "big"), oracle.g1_generator_mul(5), C.byref(s)) == 0
        assert ok.value is True
    finally:
        K.set_mode(start)


def test_verifier_host_steps(K, oracle, oracle_setup):
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle, oracle_setup)
    rnd = random.Random(15)
    n = 3
    items = [_opening(oracle, rnd) for _ in range(n)]

    def be(x):
        return int(x).to_bytes(32, "big")

    def blocks(items):
        records = b"".join(cm + be(z) + be(y) + pi for cm, z, y, pi in items)
        r = int.from_bytes(E.batch_r_eth(records), "big")
        sums, ysum, rp = [(bytes(96), True)] * 3, 0, 1
        for cm, z, y, pi in items:
            (pxy, pinf), (cxy, cinf) = oracle.g1_decompress(pi), oracle.g1_decompress(cm)
            for k, (xy, inf, sc) in enumerate(((pxy, pinf, rp), (pxy, pinf, rp * z % R), (cxy, cinf, rp))):
                t = (bytes(96), True) if inf or sc == 0 else oracle.g1_mul_affine(xy, sc)
                sums[k] = oracle.g1_add_affine(sums[k][0], sums[k][1], t[0], t[1])
            ysum = (ysum + rp * y) % R
            rp = rp * r % R
        sums97 = b"".join((b"\x01" + bytes(96)) if inf else (b"\x00" + xy) for xy, inf in sums)
        return records, r, sums97, ysum

    records, r, sums97, ysum = blocks(items)
    res = capi.verifier_host_steps(records, n, NONE_BAD, sums97, be(ysum), C.byref(s), ETH)
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 1, NONE_BAD)
    assert bytes(res.r) == E.batch_r_eth(records) == be(r)
    # the same records under the other modes' headers give another r
    assert bytes(capi.verifier_host_steps(records, n, NONE_BAD, sums97, be(ysum), C.byref(s), 0).r) != be(r)
    # one y altered: not ok
    cm, z, y, pi = items[1]
    wrong = list(items)
    wrong[1] = (cm, z, (y + 1) % R, pi)
    records2, r2, sums2, ysum2 = blocks(wrong)
    res = capi.verifier_host_steps(records2, n, NONE_BAD, sums2, be(ysum2), C.byref(s), ETH)
    assert (res.state, res.rc, res.ok) == (1, 0, 0) and bytes(res.r) == be(r2) and r2 != r
    # the empty batch (three sums at infinity, sum r^i y_i = 0) verifies, as in c-kzg mode, and its r is the header's digest alone
    res = capi.verifier_host_steps(None, 0, NONE_BAD, (b"\x01" + bytes(96)) * 3, bytes(32), C.byref(s), ETH)
    assert (res.state, res.rc, res.ok) == (1, 0, 1) and bytes(res.r) == E.batch_r_eth(b"")
    # a rejected input answers C_KZG_BADARGS
    res = capi.verifier_host_steps(None, n, 1, None, None, C.byref(s), ETH)
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, 1)
