"""CPU: the parts of the asynchronous cell verifier (lwkzg_cell_verifier_*) that need no GPU. The new symbols in
the header, the export list and the binding; the argument checks of new and enqueue; the slot hash and the compare of the grouping
kernels compiled for the host and run through a sequential emulation of the kernels against a plain map (tests/cell_group_check.hip);
and the two host steps of an enqueue through the host-only hook, on a batch whose digests, sums and interpolant commitment come from
tests/cell_verify_spec.py and the CPU oracle and whose KZGSettings is put together by hand (G2 and [tau^64]G2)."""
import ctypes as C
import hashlib
import os
import re
import shutil
import struct
import subprocess

import pytest

import cell_verify_spec as V
import cells_spec as S
from conftest import R, ROOT, TAU
from test_gpu_cell_verify import Poly

NEW_SYMBOLS = ["lwkzg_cell_verifier_new", "lwkzg_cell_verifier_enqueue", "lwkzg_cell_verifier_wait", "lwkzg_cell_verifier_host_steps",
               "lwkzg_cell_group_device"]
NONE_BAD = 0xffffffff
MODES = [S.MODE_REFERENCE, S.MODE_CKZG]


def test_new_symbols_are_declared_exported_and_bound(K):
    from lambdaworks_kzg_amd import capi
    header = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    l = K.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bC_KZG_RET %s\(" % name, header), name
    assert re.search(r"\bint\s+lwkzg_cell_verifier_pending\(", header) and re.search(r"\bvoid\s+lwkzg_cell_verifier_free\(", header)
    for name in NEW_SYMBOLS + ["lwkzg_cell_verifier_pending", "lwkzg_cell_verifier_free"]:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(l, name), name
    assert C.sizeof(K.CellVerifyResult) == 20 + capi.CELL_VERIFY_PARTIAL_BYTES and K.CellVerifyResult.partials.offset == 20
    assert "uint8_t  partials[LWKZG_CELL_VERIFY_PARTIAL_BYTES]" in header
    for method in ("enqueue", "pending", "wait", "free"):
        assert hasattr(K.CellVerifier, method), method
    # the blob verifier's header comment no longer names the cell verifications as a gap
    assert "de-duplicate commitments on the\n * host mid-call)" not in header


def test_argument_checks_need_no_gpu(K):
    l = K.lib()
    res = K.CellVerifyResult()
    assert l.lwkzg_cell_verifier_enqueue(None, C.byref(res), None, None, None, None, 0, None) == K.C_KZG_BADARGS
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, NONE_BAD)
    assert l.lwkzg_cell_verifier_enqueue(None, None, None, None, None, None, 0, None) == K.C_KZG_BADARGS
    h = C.c_void_p(5)
    assert l.lwkzg_cell_verifier_new(C.byref(h), None, 64) == K.C_KZG_BADARGS and not h.value
    assert l.lwkzg_cell_verifier_new(None, None, 64) == K.C_KZG_BADARGS
    s = K.KZGSettings()
    s.fs = s.g1_values = s.g2_values = None
    assert l.lwkzg_cell_verifier_new(C.byref(h), C.byref(s), 0) == K.C_KZG_BADARGS and not h.value
    assert l.lwkzg_cell_verifier_pending(None) == -1 and l.lwkzg_cell_verifier_wait(None) == K.C_KZG_BADARGS
    l.lwkzg_cell_verifier_free(None)
    u32 = C.c_uint32
    assert l.lwkzg_cell_group_device(None, None, None, None, None, None, None, None, None, None, None, 4, 1, 0xffffffff, None) == K.C_KZG_BADARGS
    one = (u32 * 2)()
    assert l.lwkzg_cell_group_device(one, one, C.create_string_buffer(48), one, one, one, one, (u32 * 129)(), one, None, None, 0, 1,
                                     0xffffffff, None) == K.C_KZG_BADARGS


def test_slot_hash_and_compare_on_the_host(tmp_path):
    """tests/cell_group_check.hip: cell_group.cuh compiled for the host; insert, scan and sort emulated lane after lane in a shuffled
    order against a plain map, with every key on one chain (mask 0), on two (mask 1) and spread"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "cell_group_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-I", os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cell_group_check.hip"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("ok: 412 cases"), out


def _hand_built_settings(capi, oracle):
    """fs and g1_values NULL; g2_values: 65 entries of which [0] = G2 and [64] = [tau^64]G2 are filled (all the cell check reads)"""
    def blst_fp(be48):
        return struct.pack("<6Q", *[int.from_bytes(be48[8 * k:8 * k + 8], "big") for k in range(6)])

    def g2(k):
        xy = oracle.g2_generator_mul(k)
        return b"".join(blst_fp(xy[48 * j:48 * j + 48]) for j in range(4)) + blst_fp((1).to_bytes(48, "big")) + blst_fp(bytes(48))

    blob = g2(1) + bytes(288 * 63) + g2(pow(TAU, 64, R))
    keep = C.create_string_buffer(blob, len(blob))
    s = capi.KZGSettings()
    s.fs, s.g1_values, s.g2_values = None, None, C.addressof(keep)
    return s, keep


def _flag_xy(point):
    xy, inf = point
    return (b"\x01" + bytes(96)) if inf else (b"\x00" + xy)


def _blocks(oracle, items, mode):
    """what the device sends down for an honest batch, from the restatement: distinct, digests, first_item, P | RLP | RLC, RLI"""
    distinct, rows = V.dedupe([it[0] for it in items])
    digests = b"".join(V.item_digest(row, k, cell, proof) for row, (_, k, cell, proof) in zip(rows, items))
    first_item = [rows.index(j) for j in range(len(distinct))]
    r, p_sum, rlc, rli, rlp = V.sums(oracle, items, mode, TAU)
    sums97 = _flag_xy(p_sum) + _flag_xy(rlp) + _flag_xy(rlc)
    return distinct, digests, first_item, sums97, oracle.g1_compress(*rli), p_sum, rlp


@pytest.fixture(scope="module")
def honest(oracle):
    """five items over two polynomials, one commitment three times and an item twice -- per mode"""
    out = {}
    for mode in MODES:
        a, b = Poly.seeded(oracle, 3000), Poly.seeded(oracle, 3001)
        items = [a.item(5, mode), b.item(5, mode), a.item(64, mode), b.item(5, mode), a.item(127, mode)]
        out[mode] = (items,) + _blocks(oracle, items, mode)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_host_steps_honest_and_one_corrupted_sum(K, oracle, honest, mode):
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle)
    items, distinct, digests, first_item, sums97, rli48, p_sum, rlp = honest[mode]
    n, m = len(items), len(distinct)
    assert (n, m, first_item) == (5, 2, [0, 1])
    clean = [0] * (2 * n)
    res = capi.cell_verifier_host_steps(b"".join(distinct), m, digests, n, NONE_BAD, clean, first_item, sums97, rli48, C.byref(s), mode)
    assert (res.state, res.rc, res.ok, res.first_bad, res.m) == (1, 0, 1, NONE_BAD, m)
    assert bytes(res.partials) == V.partials_bytes(oracle, items, mode, TAU)
    assert V.verdict_known_tau(oracle, items, mode, TAU) is True
    # one sum corrupted (RLP in P's place): the call answers, the answer is false, the partials say what was summed
    wrong = _flag_xy(rlp) + sums97[97:]
    res = capi.cell_verifier_host_steps(b"".join(distinct), m, digests, n, NONE_BAD, clean, first_item, wrong, rli48, C.byref(s), mode)
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, 0, 0, NONE_BAD)
    assert bytes(res.partials)[:32] == V.partials_bytes(oracle, items, mode, TAU)[:32] and bytes(res.partials)[32:129] == _flag_xy(rlp)
    # one digest altered: r is the hash of what came down (the sums are the device's business: given as before, they still balance)
    altered = digests[:-1] + bytes([digests[-1] ^ 1])
    res = capi.cell_verifier_host_steps(b"".join(distinct), m, altered, n, NONE_BAD, clean, first_item, sums97, rli48, C.byref(s), mode)
    msg = V.DOMAIN + struct.pack("<QQQQ", 4096, 64, m, n) + b"".join(distinct) + altered
    r2 = int.from_bytes(hashlib.sha256(msg).digest(), "little" if mode == S.MODE_CKZG else "big") % R
    assert (res.state, res.rc) == (1, 0) and bytes(res.partials)[:32] == S.to_bytes(r2, mode)
    assert bytes(res.partials)[:32] != V.partials_bytes(oracle, items, mode, TAU)[:32]
    # a flag byte that is neither 0 nor 1 is an answer too (as lwkzg_verifier_host_steps'); an unknown mode is the hook's own BADARGS
    res = capi.cell_verifier_host_steps(b"".join(distinct), m, digests, n, NONE_BAD, clean, first_item, b"\x02" + sums97[1:], rli48, C.byref(s), mode)
    assert (res.state, res.rc, res.ok) == (1, K.C_KZG_BADARGS, 0) and bytes(res.partials) == bytes(capi.CELL_VERIFY_PARTIAL_BYTES)
    with pytest.raises(K.KzgError):
        capi.cell_verifier_host_steps(b"".join(distinct), m, digests, n, NONE_BAD, clean, first_item, sums97, rli48, C.byref(s), 7)
    del keep


@pytest.mark.parametrize("mode", MODES)
def test_host_steps_rejections_and_first_bad(K, oracle, mode):
    """a rejected batch reads nothing behind what decides it: no commitments, digests or sums are given"""
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle)
    n, m = 9, 3
    first_item = [0, 2, 5]                        # the third distinct commitment is first seen at item 5
    mode_code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR

    def steps(bad_index, status):
        res = capi.cell_verifier_host_steps(None, m, None, n, bad_index, status, first_item if status is not None else None, None, None,
                                            C.byref(s), mode)
        assert res.state == 1 and res.ok == 0 and bytes(res.partials) == bytes(capi.CELL_VERIFY_PARTIAL_BYTES)
        return res.rc, res.first_bad

    def words(items=(), commitments=()):
        w = [0] * (2 * n)
        for i in items:
            w[i] = mode_code
        for j in commitments:
            w[n + j] = mode_code
        return w

    # an index >= 128: BADARGS in both modes, decided first, whatever else is wrong, and without the words
    assert steps(6, None) == (K.C_KZG_BADARGS, 6)
    assert steps(6, words(items=[1], commitments=[0])) == (K.C_KZG_BADARGS, 6)
    assert steps(0, words()) == (K.C_KZG_BADARGS, 0)
    # a status word: the mode's code at the lowest item at fault
    assert steps(NONE_BAD, words(items=[7])) == (mode_code, 7)
    assert steps(NONE_BAD, words(items=[8, 3])) == (mode_code, 3)
    # a bad commitment counts at the item it was first seen at: 5, before the bad proof at 7 ...
    assert steps(NONE_BAD, words(items=[7], commitments=[2])) == (mode_code, 5)
    # ... and behind a bad proof at 4
    assert steps(NONE_BAD, words(items=[4], commitments=[2])) == (mode_code, 4)
    assert steps(NONE_BAD, words(commitments=[1, 2])) == (mode_code, 2)
    assert steps(NONE_BAD, words(commitments=[0])) == (mode_code, 0)
    # the words behind the m-th commitment are padding's: never read
    w = words()
    w[n + m] = mode_code
    with pytest.raises(K.KzgError) as e:          # (clean, so the batch is honest and its blocks are missing)
        capi.cell_verifier_host_steps(None, m, None, n, NONE_BAD, w, first_item, None, None, C.byref(s), mode)
    assert e.value.rc == K.C_KZG_BADARGS
    del keep
