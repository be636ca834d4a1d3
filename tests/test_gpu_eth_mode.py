"""GPU: the consensus-specs mode (LWKZG_MODE_ETH) on the blob side -- commitments on every engine form, the range rule, the three proof
calls, every proof schedule, blob verification in all its forms, per-item opening verification, the cost of switching and the
multi-device calls. Expected values: the CPU oracle's c-kzg mode on byte-reversed inputs for a handful of blobs (independent code), the
consensus specs' transcripts restated with hashlib (tests/eth_spec.py), and -- to carry those across launch shapes -- the library's own
c-kzg mode on byte-reversed inputs (tests/eth_spec.py has the identities)."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import blobs as B
import eth_spec as E
from conftest import R, ROOT, SETUP_PATH

pytestmark = pytest.mark.gpu

ETH, LAG, MONO = 2, 2, 1
BLOB = B.BYTES_PER_BLOB
NONE_BAD = 0xffffffff
ZERO_BLOB = bytes(BLOB)
RM1_BLOB = (R - 1).to_bytes(32, "big") * 4096
ODD_INF = bytes([0xc0, 0x01]) + bytes(46)     # infinity with a stray bit: valid, not canonical
INF = bytes([0xc0]) + bytes(47)
OMEGA = pow(7, (R - 1) // 4096, R)
_cache = {}


def syn(i):
    return B.synthetic_blob(81000 + i)        # big-endian canonical elements


@pytest.fixture(scope="module")
def ts(K):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    t = K.TrustedSetup.from_file(SETUP_PATH)
    t.enable_direct_table_forms(10, LAG)
    yield t
    t.free()


def _tables(ts, form):
    if form == "bucket":
        ts.enable_direct_table(0)
    else:
        ts.enable_direct_table_forms(10, LAG if form == "lag" else MONO)
        assert ts.direct_table_forms() == (LAG if form == "lag" else MONO)


@contextlib.contextmanager
def eth(ts, form="lag"):
    """the settings in eth mode on the named table form; afterwards the mode is handed back and the module's tables restored"""
    _tables(ts, form)
    ts.set_mode(ETH)
    try:
        yield ts
    finally:
        ts.set_mode(-1)
        _tables(ts, "lag")


def as_ckzg(ts, fn):
    """fn() with the settings in c-kzg mode (both modes run on the same tables: nothing moves), then back to eth mode"""
    ts.set_mode(1)
    try:
        return fn()
    finally:
        ts.set_mode(ETH)


def dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def host(t):
    return bytes(t.cpu().numpy().tobytes())


def split(raw, size):
    return [raw[size * i:size * i + size] for i in range(len(raw) // size)]


def _oracle_commit(oracle, oracle_setup, blob):
    key = ("oc", blob[:64], blob[-64:])
    if key not in _cache:
        rc, c = oracle.blob_to_kzg_commitment(E.rev32(blob), oracle_setup, oracle.MODE_C)
        assert rc == 0
        _cache[key] = c
    return _cache[key]


def _big(K, ts):
    """1025 honest (blob, commitment, z, y, proof) in eth mode's bytes, made ONCE through identity (3): commitments and openings by the
    library's c-kzg mode on the reversed blobs, z from hashlib; blob 0 is the zero blob (its commitment the canonical infinity)"""
    if "big" not in _cache:
        n = 1025
        blobs = [ZERO_BLOB] + [syn(100 + i) for i in range(1, n)]
        data = b"".join(blobs)
        rdata = E.rev32(data)
        comms = as_ckzg(ts, lambda: K.blob_to_kzg_commitment_batch(rdata, ts))
        assert comms[0] == INF
        zs = [E.challenge_eth(b, c) for b, c in zip(blobs, comms)]
        opened = as_ckzg(ts, lambda: K.compute_kzg_proof_batch(rdata, E.rev32(b"".join(zs)), ts))
        _cache["big"] = dict(n=n, blobs=blobs, data=data, comms=comms, zs=zs, proofs=[p for p, _ in opened], ys=[y[::-1] for _, y in opened])
    return _cache["big"]


def _records(big, idx):
    return b"".join(big["comms"][i] + big["zs"][i] + big["ys"][i] + big["proofs"][i] for i in idx)


@pytest.mark.parametrize("form", ["lag", "mono", "bucket"])
def test_commitments_on_each_engine_form(K, ts, oracle, oracle_setup, form):
    import torch
    blobs = [ZERO_BLOB, RM1_BLOB] + [syn(i) for i in range(7)]
    data = b"".join(blobs)
    with eth(ts, form):
        want = as_ckzg(ts, lambda: K.blob_to_kzg_commitment_batch(E.rev32(data), ts))      # identity (3), on the same tables
        for i in range(3):                                                                     # ... anchored at the oracle
            assert want[i] == _oracle_commit(oracle, oracle_setup, blobs[i]), i
        assert want[0] == INF
        rc, other = oracle.blob_to_kzg_commitment(blobs[2], oracle_setup, oracle.MODE_R)       # (the same bytes read as coefficients: another point)
        assert rc == 0 and other != want[2]
        for i in range(3):
            assert K.blob_to_kzg_commitment(blobs[i], ts) == want[i], i                       # n = 1, host
        assert K.blob_to_kzg_commitment_batch(data, ts) == want                                # n = 9, host
        d_in = dev(data)
        for n in (1, 9):
            out = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
            st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
            K.blob_to_kzg_commitment_batch_device(out.data_ptr(), d_in.data_ptr() + (2 * BLOB if n == 1 else 0), n, ts, None, st.data_ptr())
            torch.cuda.synchronize()
            assert split(host(out), 48) == (want[2:3] if n == 1 else want) and st.tolist() == [0] * n, n


@pytest.mark.parametrize("form", ["lag", "mono"])
def test_range_rule(K, ts, form):
    """`ff 00 .. 00` is >= r read big-endian (and 255 read little-endian): rejected; `00 .. 00 ff` is 255: accepted; r itself: rejected"""
    import torch
    n = 3
    base = [syn(20 + i) for i in range(n)]
    places = [(0, 0), (n - 1, 5), (1, 4095)]

    def put(blobs, j, e, elem):
        b = bytearray(blobs[j])
        b[32 * e:32 * e + 32] = elem
        return blobs[:j] + [bytes(b)] + blobs[j + 1:]

    with eth(ts, form):
        out, bad = C.create_string_buffer(48 * n), C.c_size_t(99)
        for j, e in places:
            for elem in (b"\xff" + bytes(31), R.to_bytes(32, "big")):
                data = b"".join(put(base, j, e, elem))
                assert K.lib().lwkzg_blob_to_kzg_commitment_batch(out, data, n, ts.ref(), C.byref(bad)) == K.C_KZG_BADARGS
                assert bad.value == j
                d_in, d_out = dev(data), torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
                st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
                K.blob_to_kzg_commitment_batch_device(d_out.data_ptr(), d_in.data_ptr(), n, ts, None, st.data_ptr())
                torch.cuda.synchronize()
                assert st.tolist() == [K.C_KZG_BADARGS if i == j else 0 for i in range(n)], (j, e)
        good = base
        for j, e in places:
            good = put(good, j, e, bytes(31) + b"\xff")
        data = b"".join(good)
        got = K.blob_to_kzg_commitment_batch(data, ts)
        assert got == as_ckzg(ts, lambda: K.blob_to_kzg_commitment_batch(E.rev32(data), ts))
        assert got != K.blob_to_kzg_commitment_batch(b"".join(base), ts)


@pytest.mark.parametrize("form", ["lag", "mono"])
def test_compute_kzg_proof(K, ts, oracle, oracle_setup, form):
    blob = syn(30)
    elems = B.blob_scalars(blob, big_endian=True)
    k = 5
    on_domain = pow(OMEGA, int(format(k, "012b")[::-1], 2), R)      # the domain point of element k: w^bitrev12(k)
    with eth(ts, form):
        for z in (0x1234567 * 0x89abcdef % R, on_domain):
            zb = z.to_bytes(32, "big")
            proof, y = K.compute_kzg_proof(blob, zb, ts)
            rc, want_p, want_y = oracle.compute_kzg_proof(E.rev32(blob), zb[::-1], oracle_setup, oracle.MODE_C)
            assert rc == 0 and (proof, y) == (want_p, want_y[::-1]), hex(z)
        assert int.from_bytes(y, "big") == elems[k]                  # (the in-domain branch: y is the blob's own element)
        for z in (R, 2 ** 256 - 1):
            with pytest.raises(K.KzgError) as e:
                K.compute_kzg_proof(blob, z.to_bytes(32, "big"), ts)
            assert e.value.rc == K.C_KZG_BADARGS


def test_blob_proofs_against_the_oracle(K, ts, oracle, oracle_setup):
    import torch
    from lambdaworks_kzg_amd import capi
    blobs = [ZERO_BLOB, syn(40), syn(41)]
    n = len(blobs)
    data = b"".join(blobs)
    with eth(ts):
        canon = K.blob_to_kzg_commitment_batch(data, ts)
        given = [ODD_INF] + canon[1:]
        zs = [E.challenge_eth(b, c) for b, c in zip(blobs, canon)]                      # (a non-canonical infinity is re-hashed over the canonical bytes)
        want = []
        for b, z in zip(blobs, zs):
            rc, p, _ = oracle.compute_kzg_proof(E.rev32(b), z[::-1], oracle_setup, oracle.MODE_C)
            assert rc == 0
            want.append(p)
        rc, not_this = oracle.compute_blob_kzg_proof(E.rev32(blobs[1]), canon[1], oracle_setup, oracle.MODE_C)   # c-kzg's own transcript: another proof
        assert rc == 0 and not_this != want[1]
        assert [K.compute_blob_kzg_proof(b, c, ts) for b, c in zip(blobs, given)] == want
        assert K.compute_blob_kzg_proof_batch(data, b"".join(given), ts) == want
        d_b, d_c = dev(data), dev(b"".join(given))
        d_p, d_cm = torch.zeros(48 * n, dtype=torch.uint8, device="cuda"), torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        K.compute_blob_kzg_proof_batch_device(d_p.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), n, ts, None, st.data_ptr())
        torch.cuda.synchronize()
        assert split(host(d_p), 48) == want and st.tolist() == [0] * n
        d_p.zero_()
        K.commit_and_prove_batch_device(d_cm.data_ptr(), d_p.data_ptr(), d_b.data_ptr(), n, ts, None, st.data_ptr())
        torch.cuda.synchronize()
        assert split(host(d_cm), 48) == canon and split(host(d_p), 48) == want and st.tolist() == [0] * n
        # the challenges themselves: 32 big-endian bytes, the consensus specs' message
        d_z, d_canon = torch.zeros(32 * n, dtype=torch.uint8, device="cuda"), dev(b"".join(canon))
        capi.compute_challenges_device(d_z.data_ptr(), d_b.data_ptr(), d_canon.data_ptr(), n, ts)
        torch.cuda.synchronize()
        assert split(host(d_z), 32) == zs
        d_rb = dev(E.rev32(data))
        z_ckzg = as_ckzg(ts, lambda: (capi.compute_challenges_device(d_z.data_ptr(), d_rb.data_ptr(), d_canon.data_ptr(), n, ts), torch.cuda.synchronize(),
                                      split(host(d_z), 32))[2])
        assert all(a != b and a != b[::-1] for a, b in zip(zs, z_ckzg))


def test_blob_proofs_across_the_launch_shapes(K, ts):
    """n = 1, 9, 65, 193, 385, 1025: the cooperative path, the small-host limit, the pipelined mid-size minimum, the mid-host limit, the chunk"""
    import torch
    from lambdaworks_kzg_amd import capi
    with eth(ts):
        big = _big(K, ts)
        d_b, d_c = dev(big["data"]), dev(b"".join(big["comms"]))
        total = big["n"]
        d_cm = torch.zeros(48 * total, dtype=torch.uint8, device="cuda")
        K.blob_to_kzg_commitment_batch_device(d_cm.data_ptr(), d_b.data_ptr(), total, ts)
        torch.cuda.synchronize()
        assert split(host(d_cm), 48) == big["comms"]
        ts.reserve(total)
        seen = set()
        for n in (1, 9, 65, 193, 385, 1025):
            d_p = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
            st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
            K.compute_blob_kzg_proof_batch_device(d_p.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), n, ts, None, st.data_ptr())
            torch.cuda.synchronize()
            seen.add(capi.last_proof_schedule())
            assert int(st.abs().sum().item()) == 0, n
            assert split(host(d_p), 48) == big["proofs"][:n], n
            d_p.zero_()
            K.commit_and_prove_batch_device(d_cm.data_ptr(), d_p.data_ptr(), d_b.data_ptr(), n, ts, None, st.data_ptr())
            torch.cuda.synchronize()
            assert split(host(d_p), 48) == big["proofs"][:n] and split(host(d_cm), 48)[:n] == big["comms"][:n], n
        assert len(seen) >= 2, seen


_WORKER = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, blobs as B, lambdaworks_kzg_amd as K
from lambdaworks_kzg_amd import capi
ts = K.TrustedSetup.from_file(%r)
ts.set_mode(2)
n = 256
blobs = [B.synthetic_blob(92000 + i) for i in range(n)]
blobs[7] = bytes(B.BYTES_PER_BLOB)
data = b"".join(blobs)
comms = K.blob_to_kzg_commitment_batch(data, ts)
canon7 = comms[7]
comms[7] = bytes([0xc0, 0x01]) + bytes(46)          # infinity with a stray bit: valid, not canonical
d_b = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
d_c = torch.frombuffer(bytearray(b"".join(comms)), dtype=torch.uint8).cuda()
d_o = torch.empty(48 * n, dtype=torch.uint8, device="cuda"); d_s = torch.zeros(n, dtype=torch.int32, device="cuda")
ts.reserve(n)
took = []
for rep in range(2):
    K.compute_blob_kzg_proof_batch_device(d_o.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), n, ts, None, d_s.data_ptr())
    torch.cuda.synchronize(); took.append(capi.last_proof_schedule())
print(json.dumps({"took": took, "status": int(d_s.abs().sum().item()), "proofs": bytes(d_o.cpu().numpy().tobytes()).hex(),
                  "comms": [comms[0].hex(), canon7.hex(), comms[255].hex()]}))
"""


def _run(**env):
    code = _WORKER % (ROOT, os.path.join(ROOT, "tests", "golden"), SETUP_PATH)
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, **env), timeout=600).decode()
    return json.loads(out.strip().splitlines()[-1])


def test_every_schedule_once(K, oracle, oracle_setup):
    """the same 256 blobs in eth mode, a fresh process per run, one after the other (a failing process ends the loop: check_output raises)"""
    default = _run()
    assert default["status"] == 0
    for k in range(5):
        r = _run(LWKZG_EXPERIMENTAL="1", LWKZG_PROOF_SCHEDULE=str(k))
        assert r["took"] == [k, k], (k, r["took"])
        assert r["status"] == 0 and r["proofs"] == default["proofs"], k
    proofs = bytes.fromhex(default["proofs"])
    for j, i in enumerate((0, 7, 255)):
        blob = ZERO_BLOB if i == 7 else B.synthetic_blob(92000 + i)
        cm = bytes.fromhex(default["comms"][j])
        assert cm == _oracle_commit(oracle, oracle_setup, blob)
        rc, want, _ = oracle.compute_kzg_proof(E.rev32(blob), E.challenge_eth(blob, cm)[::-1], oracle_setup, oracle.MODE_C)
        assert rc == 0 and proofs[48 * i:48 * i + 48] == want, i


def _verify_all_forms(K, ts, multi, blobs, comms, proofs):
    """(host batch, device batch, verifier result, two shards on one settings object, lwkzg_multi_* over two contexts of device 0) for one batch"""
    import torch
    n = len(comms)
    data, cm, pf = b"".join(blobs), b"".join(comms), b"".join(proofs)
    d_b, d_c, d_p = dev(data), dev(cm), dev(pf)
    out = {"host": K.verify_blob_kzg_proof_batch(data, cm, pf, n, ts),
           "device": K.verify_blob_kzg_proof_batch_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n, ts),
           "multi": multi.verify_blob_kzg_proof_batch(data, cm, pf, n)}
    v = K.Verifier(ts, max(n, 1))
    try:
        res = v.enqueue(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n)
        v.wait()
        out["verifier"] = res
    finally:
        v.free()
    k = n - n // 2
    shards = [K.VerifyShard(b"".join(blobs[:k]), b"".join(comms[:k]), b"".join(proofs[:k]), k, ts),
              K.VerifyShard(b"".join(blobs[k:]), b"".join(comms[k:]), b"".join(proofs[k:]), n - k, ts)]
    try:
        records = shards[0].records + shards[1].records
        out["records"] = records
        out["sharded"] = K.verify_shards_finish(shards[0].partial(records, n, 0) + shards[1].partial(records, n, k), 2, n, ts)
    finally:
        for s in shards:
            s.free()
    torch.cuda.synchronize()
    return out


def test_blob_verification(K, ts):
    import torch
    from lambdaworks_kzg_amd import capi
    multi = capi.MultiSetup.from_file(SETUP_PATH, [0, 0])      # device 0 named twice: n = 1 leaves one context an empty shard
    try:
        multi.enable_direct_table(10)
        multi.set_mode(ETH)
        _blob_verification(K, ts, multi)
    finally:
        multi.free()


def _blob_verification(K, ts, multi):
    import torch
    with eth(ts):
        big = _big(K, ts)
        for n in (1, 3, 65):
            idx = list(range(1, n + 1)) if n < 65 else list(range(n))             # (65: with the zero blob and its commitment at infinity)
            blobs, comms, proofs = ([big[key][i] for i in idx] for key in ("blobs", "comms", "proofs"))
            got = _verify_all_forms(K, ts, multi, blobs, comms, proofs)
            res = got["verifier"]
            assert got["host"] is True and got["device"] is True and got["sharded"] is True and got["multi"] is True, n
            assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 1, NONE_BAD), n
            assert got["records"] == _records(big, idx), n                        # C | z | y | proof, z and y big-endian
            assert bytes(res.r) == E.batch_r_eth(got["records"]), n
            if n == 1:
                assert K.verify_blob_kzg_proof(blobs[0], comms[0], proofs[0], ts) is True
        # n = 3: one tampered proof byte in the middle item (the sign bit: still a point of the group) -> false, rc OK
        idx = [1, 2, 3]
        blobs, comms, proofs = ([big[key][i] for i in idx] for key in ("blobs", "comms", "proofs"))
        bad = [proofs[0], bytes([proofs[1][0] ^ 0x20]) + proofs[1][1:], proofs[2]]
        got = _verify_all_forms(K, ts, multi, blobs, comms, bad)
        res = got["verifier"]
        assert got["host"] is False and got["device"] is False and got["sharded"] is False and got["multi"] is False
        assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 0, NONE_BAD)
        assert K.verify_blob_kzg_proof(blobs[1], comms[1], bad[1], ts) is False
        each = K.verify_blob_kzg_proof_each(b"".join(blobs), b"".join(comms), b"".join(bad), ts)
        assert each == [(0, True), (0, False), (0, True)]
        # a non-canonical element in one blob: C_KZG_BADARGS, and the verifier names the item
        nc = bytearray(blobs[2])
        nc[32 * 9:32 * 9 + 32] = b"\xff" + bytes(31)
        blobs_nc = [blobs[0], blobs[1], bytes(nc)]
        ok = C.c_bool(True)
        assert K.lib().verify_blob_kzg_proof_batch(C.byref(ok), b"".join(blobs_nc), b"".join(comms), b"".join(proofs), 3, ts.ref()) == K.C_KZG_BADARGS
        d_b, d_c, d_p = dev(b"".join(blobs_nc)), dev(b"".join(comms)), dev(b"".join(proofs))
        assert K.lib().lwkzg_verify_blob_kzg_proof_batch_device(C.byref(ok), d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), 3, ts.ref(), None) == K.C_KZG_BADARGS
        v = K.Verifier(ts, 3)
        try:
            res = v.enqueue(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), 3)
            v.wait()
            assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, 2)
            res = v.enqueue(None, None, None, 0)                                  # the empty batch verifies
            v.wait()
            assert (res.state, res.rc, res.ok) == (1, 0, 1)
        finally:
            v.free()
        each = K.verify_blob_kzg_proof_each(b"".join(blobs_nc), b"".join(comms), b"".join(proofs), ts)
        assert each == [(0, True), (0, True), (K.C_KZG_BADARGS, False)]
        assert K.verify_blob_kzg_proof_batch(b"", b"", b"", 0, ts) is True
        assert multi.verify_blob_kzg_proof_batch(b"", b"", b"", 0) is True
        # the cross-mode negative: c-kzg mode's proof for B' (its own challenge) presented in eth mode with B
        rblob = E.rev32(blobs[0])
        p_ckzg = as_ckzg(ts, lambda: K.compute_blob_kzg_proof(rblob, comms[0], ts))
        assert as_ckzg(ts, lambda: K.verify_blob_kzg_proof(rblob, comms[0], p_ckzg, ts)) is True
        assert p_ckzg != proofs[0]
        assert K.verify_blob_kzg_proof(blobs[0], comms[0], p_ckzg, ts) is False
        assert K.verify_blob_kzg_proof_batch(blobs[0], comms[0], p_ckzg, 1, ts) is False
        # 1025 blobs, device-resident (past the chunk) and through host pointers (the staged upload)
        d_b, d_c, d_p = dev(big["data"]), dev(b"".join(big["comms"])), dev(b"".join(big["proofs"]))
        n = big["n"]
        assert K.verify_blob_kzg_proof_batch_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n, ts) is True
        assert K.verify_blob_kzg_proof_batch(big["data"], b"".join(big["comms"]), b"".join(big["proofs"]), n, ts) is True
        flipped = list(big["proofs"])
        flipped[1000] = bytes([flipped[1000][0] ^ 0x20]) + flipped[1000][1:]
        d_p2 = dev(b"".join(flipped))
        assert K.verify_blob_kzg_proof_batch_device(d_b.data_ptr(), d_c.data_ptr(), d_p2.data_ptr(), n, ts) is False
        torch.cuda.synchronize()


def test_verify_kzg_proof_each(K, ts):
    with eth(ts):
        big = _big(K, ts)
        idx = [1, 2, 3]
        comms, zs, ys, proofs = ([big[key][i] for i in idx] for key in ("comms", "zs", "ys", "proofs"))
        for i in range(3):
            assert K.verify_kzg_proof(comms[i], zs[i], ys[i], proofs[i], ts) is True
        ys2 = [ys[0], ((int.from_bytes(ys[1], "big") + 1) % R).to_bytes(32, "big"), ys[2]]
        zs2 = [zs[0], zs[1], R.to_bytes(32, "big")]
        got = K.verify_kzg_proof_each(b"".join(comms), b"".join(zs2), b"".join(ys2), b"".join(proofs), ts)
        assert got == [(0, True), (0, False), (K.C_KZG_BADARGS, False)]
        with pytest.raises(K.KzgError) as e:
            K.verify_kzg_proof(comms[2], zs2[2], ys[2], proofs[2], ts)
        assert e.value.rc == K.C_KZG_BADARGS


def test_switching_cost(K, ts, oracle_setup):
    data = b"".join(syn(50 + i) for i in range(3))
    _tables(ts, "lag")
    try:
        ts.set_mode(K.MODE_CKZG)
        want = K.blob_to_kzg_commitment_batch(E.rev32(data), ts)
        forms, bits = ts.direct_table_forms(), ts.direct_table_bits()
        assert (forms, bits) == (LAG, 10)
        assert K.lib().lwkzg_settings_set_mode(ts.ref(), ETH) == K.MODE_CKZG        # returns the mode it answered in before
        assert ts.get_mode() == ETH
        assert (ts.direct_table_forms(), ts.direct_table_bits()) == (forms, bits)   # nothing moved, nothing derived
        assert K.blob_to_kzg_commitment_batch(data, ts) == want
        # a setup loaded from its Lagrange form answers in c-kzg mode at first; eth mode after the load gives the monomial load's bytes
        lag_ts = K.TrustedSetup.from_lagrange_bytes(ts.g1_lagrange(), oracle_setup.g2_compressed())
        try:
            assert lag_ts.get_mode() == K.MODE_CKZG
            assert lag_ts.set_mode(ETH) == K.MODE_CKZG
            assert K.blob_to_kzg_commitment_batch(data, lag_ts) == want
        finally:
            lag_ts.free()
    finally:
        ts.set_mode(-1)
        _tables(ts, "lag")


def test_multi(K, ts):
    """two contexts of device 0 in eth mode: commitments and blob proofs equal the single-device calls'; the batch verifies"""
    n = 5
    blobs = [syn(60 + i) for i in range(n)]
    data = b"".join(blobs)
    from lambdaworks_kzg_amd import capi
    m = capi.MultiSetup.from_file(SETUP_PATH, [0, 0])
    try:
        m.enable_direct_table(10)
        m.set_mode(ETH)
        with eth(ts):
            comms = K.blob_to_kzg_commitment_batch(data, ts)
            proofs = K.compute_blob_kzg_proof_batch(data, b"".join(comms), ts)
            assert m.blob_to_kzg_commitment_batch(data) == comms
            assert m.compute_blob_kzg_proof_batch(data, b"".join(comms)) == proofs
            assert m.verify_blob_kzg_proof_batch(data, b"".join(comms), b"".join(proofs), n) is True
            bad = [proofs[0], proofs[2]] + proofs[2:]
            assert m.verify_blob_kzg_proof_batch(data, b"".join(comms), b"".join(bad), n) is False
    finally:
        m.free()
