"""GPU: batch verification of openings (C, z, y, pi) with one pairing -- lwkzg_verify_kzg_proof_batch, its _device form, the
_partial hook and lwkzg_verify_kzg_proof_each_device. The definition under test: an item is valid exactly
when the single verify_kzg_proof accepts its encoding; the records are the blob batch's; r is lwkzg_batch_challenge_host over them;
one pairing over the three r-weighted sums. Truth per item is the single call; for validly encoded items in reference mode the
oracle's known-tau check is a second truth with no pairing code. Sizes: 1, 2, and one across the wave (63, 64, 65), the 64-term slice
of k_vmsm_accumulate (65), the 256-thread block (257) and the chunk (1025); 8193 is one above kVerifyApartMax."""
import ctypes as C
import re

import pytest

import blobs as B
import openings_cases as OC
from conftest import R, SETUP_TAU2_PATH, TAU, hx

pytestmark = pytest.mark.gpu

MODES = ["reference", "ckzg", "eth"]


def _mode(K, name):
    return {"reference": K.MODE_REFERENCE, "ckzg": K.MODE_CKZG, "eth": K.MODE_ETH}[name]


def _dev(torch, data):
    return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()


def _host(K, items, ts):
    """(rc, ok, the index the error text names) of the host form"""
    try:
        return 0, K.verify_kzg_proof_batch(*OC.columns(items), ts), None
    except K.KzgError as e:
        m = re.search(r"opening (\d+) rejected", str(e))
        return e.rc, False, int(m.group(1)) if m else None


def _device(K, torch, items, ts, stream=None):
    bufs = [_dev(torch, col) for col in OC.columns(items)]
    torch.cuda.synchronize()
    try:
        return 0, K.verify_kzg_proof_batch_device(*[b.data_ptr() for b in bufs], len(items), ts, stream), None
    except K.KzgError as e:
        m = re.search(r"opening (\d+) rejected", str(e))
        return e.rc, False, int(m.group(1)) if m else None


def _check_batch(K, torch, ts, mode, items, label):
    want = OC.expected(K, mode, OC.truth(K, ts, mode, items))
    got_h, got_d = _host(K, items, ts), _device(K, torch, items, ts)
    print("%s: n=%d want %r host %r device %r" % (label, len(items), want, got_h, got_d))
    assert got_h == want, label
    assert got_d == want, label
    return want


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize("mode_name", MODES)
def test_mixed_batches(K, gpu_setup, mode_name, n):
    """honest -> true; defects that keep every encoding valid -> the single calls' conjunction; with invalid items among them -> the
    mode's code and the lowest such index in lwkzg_last_error. Host and _device forms agree."""
    import torch
    mode = _mode(K, mode_name)
    with OC.Mode(gpu_setup, mode):
        honest = OC.draw(OC.pool(K, gpu_setup, mode), n, 300 + n)
        assert _check_batch(K, torch, gpu_setup, mode, honest, "honest") == (0, True, None)
        if n >= 2:
            items, places = OC.with_defects(K, mode, honest, OC.VERDICT_KINDS, 400 + n)
            assert _check_batch(K, torch, gpu_setup, mode, items, "valid encodings")[:2] == (0, False)
            # the zero polynomial, the stray-bit infinity and a repeated honest item alone keep the batch true
            items, _ = OC.with_defects(K, mode, honest, ["zero_poly", "inf_stray"], 500 + n)
            assert _check_batch(K, torch, gpu_setup, mode, items, "infinities") == (0, True, None)
        items, places = OC.with_defects(K, mode, honest, OC.VERDICT_KINDS[:3] + OC.CODE_KINDS + OC.VERDICT_KINDS[3:], 600 + n)
        if n == 1:   # the one item with its compression flag cleared
            c, z, y, p = honest[0]
            items = [(bytes([c[0] & 0x7f]) + c[1:], z, y, p)]
        want = _check_batch(K, torch, gpu_setup, mode, items, "every kind")
        if n >= 12 or n == 1:   # (every kind found a place; bad_c and bad_pi are refused in every mode)
            assert want[0] == OC.mode_code(K, mode) and want[2] is not None


@pytest.mark.parametrize("n", [65])
def test_both_engines(K, engine_setup, n):
    import torch
    mode = K.MODE_CKZG
    with OC.Mode(engine_setup, mode):
        honest = OC.draw(OC.pool(K, engine_setup, mode), n, 11)
        assert _check_batch(K, torch, engine_setup, mode, honest, "honest") == (0, True, None)
        items, _ = OC.with_defects(K, mode, honest, OC.VERDICT_KINDS, 12)
        assert _check_batch(K, torch, engine_setup, mode, items, "valid encodings")[:2] == (0, False)
        items, _ = OC.with_defects(K, mode, honest, OC.CODE_KINDS, 13)
        assert _check_batch(K, torch, engine_setup, mode, items, "invalid")[0] == K.C_KZG_BADARGS


def test_n1_equals_verify_kzg_proof_on_the_ckzg_suite(K, gpu_setup, vectors):
    mode = K.MODE_CKZG
    with OC.Mode(gpu_setup, mode):
        seen = 0
        for c in vectors["suites"]["verify_kzg_proof"]:
            i = c["input"]
            item = (hx(i["commitment"]), hx(i["z"]), hx(i["y"]), hx(i["proof"]))
            if [len(x) for x in item] != [48, 32, 32, 48]:
                continue
            want = OC.single(K, item, gpu_setup)
            assert want == ((K.C_KZG_BADARGS, False) if c["output"] is None else (0, c["output"]))
            assert _host(K, [item], gpu_setup)[:2] == want, i
            seen += 1
        assert seen >= 10


@pytest.mark.parametrize("mode_name", MODES)
def test_r_weights(K, gpu_setup, mode_name):
    """two items on the same (C, z, pi) with y + 1 and y - 1: an unweighted sum would cancel them"""
    import torch
    mode = _mode(K, mode_name)
    with OC.Mode(gpu_setup, mode):
        items = OC.pool(K, gpu_setup, mode)
        order = OC.order_of(K, mode)
        c, z, y, p = items[7]
        up = (c, z, ((int.from_bytes(y, order) + 1) % R).to_bytes(32, order), p)
        down = (c, z, ((int.from_bytes(y, order) - 1) % R).to_bytes(32, order), p)
        for pair in ([up, down], [down, up]):
            batch = [items[3]] + pair + [items[9]]
            assert _check_batch(K, torch, gpu_setup, mode, batch, "y+1, y-1") == (0, False, None)
        assert _check_batch(K, torch, gpu_setup, mode, [items[3], items[7], items[7], items[9]], "y, y") == (0, True, None)


@pytest.mark.parametrize("n", [65, 8193])
def test_tampered_y_at_the_ends(K, gpu_setup, n):
    import torch
    mode = K.MODE_REFERENCE
    with OC.Mode(gpu_setup, mode):
        honest = OC.draw(OC.pool(K, gpu_setup, mode), n, 900 + n)
        bufs = [_dev(torch, col) for col in OC.columns(honest)]
        torch.cuda.synchronize()
        ptrs = [b.data_ptr() for b in bufs]
        assert K.verify_kzg_proof_batch_device(*ptrs, n, gpu_setup) is True
        assert K.verify_kzg_proof_batch(*OC.columns(honest), gpu_setup) is True
        for where in (0, n - 1):
            saved = bufs[2][32 * where:32 * where + 32].clone()
            bufs[2][32 * where:32 * where + 32] = _dev(torch, OC.tamper_y(K, mode, honest[where])[2])
            torch.cuda.synchronize()
            assert K.verify_kzg_proof_batch_device(*ptrs, n, gpu_setup) is False, where
            bufs[2][32 * where:32 * where + 32] = saved
            items = list(honest)
            items[where] = OC.tamper_y(K, mode, honest[where])
            assert K.verify_kzg_proof_batch(*OC.columns(items), gpu_setup) is False, where
        torch.cuda.synchronize()
        assert K.verify_kzg_proof_batch_device(*ptrs, n, gpu_setup) is True


@pytest.mark.parametrize("mode_name", MODES)
def test_equivalence_with_the_blob_batch(K, gpu_setup, mode_name):
    """the records lwkzg_verify_shard_begin returns for a blob batch, as four columns: the same r, the same partial, the same verdict"""
    from lambdaworks_kzg_amd import capi
    mode = _mode(K, mode_name)
    n = 65
    with OC.Mode(gpu_setup, mode):
        data = B.synthetic_batch(57000 + 100 * mode, n, big_endian=mode != K.MODE_CKZG)
        cms = K.blob_to_kzg_commitment_batch(data, gpu_setup)
        prs = list(K.compute_blob_kzg_proof_batch(data, b"".join(cms), gpu_setup))
        for tampered in (False, True):
            if tampered:
                prs[40] = prs[41]
            cj, pj = b"".join(cms), b"".join(prs)
            shard = capi.VerifyShard(data, cj, pj, n, gpu_setup)
            try:
                rec = shard.records
                want_partial = shard.partial(rec, n, 0)
            finally:
                shard.free()
            items = [(rec[160 * i:160 * i + 48], rec[160 * i + 48:160 * i + 80], rec[160 * i + 80:160 * i + 112], rec[160 * i + 112:160 * i + 160])
                     for i in range(n)]
            r, partial = K.verify_kzg_proof_batch_partial(*OC.columns(items), gpu_setup)
            assert r == K.batch_challenge_host(rec, n, mode)
            assert partial == want_partial
            verdict = K.verify_blob_kzg_proof_batch(data, cj, pj, n, gpu_setup)
            assert verdict is (not tampered)
            assert K.verify_kzg_proof_batch(*OC.columns(items), gpu_setup) is verdict
            assert K.verify_shards_finish(partial, 1, n, gpu_setup) is verdict


def test_non_canonical_scalars_in_reference_mode(K, gpu_setup):
    """z + r and y + r answer as z and y do, and the records hold the reduced bytes: the same r"""
    mode = K.MODE_REFERENCE
    with OC.Mode(gpu_setup, mode):
        items = OC.draw(OC.pool(K, gpu_setup, mode), 65, 41)
        items[64] = OC.tamper_y(K, mode, items[64])
        for tampered in (False, True):
            batch = items if tampered else items[:64]
            lifted = list(batch)
            for i in (0, 5, 63):
                c, z, y, p = batch[i]
                lifted[i] = (c, (int.from_bytes(z, "big") + R).to_bytes(32, "big"), (int.from_bytes(y, "big") + R).to_bytes(32, "big"), p)
            assert K.verify_kzg_proof_batch_partial(*OC.columns(lifted), gpu_setup) == K.verify_kzg_proof_batch_partial(*OC.columns(batch), gpu_setup)
            assert K.verify_kzg_proof_batch(*OC.columns(lifted), gpu_setup) is (not tampered)
            assert K.verify_kzg_proof_batch(*OC.columns(batch), gpu_setup) is (not tampered)


@pytest.mark.parametrize("mode_name", MODES)
def test_a_non_canonical_infinity_hashes_as_the_canonical_one(K, gpu_setup, mode_name):
    mode = _mode(K, mode_name)
    with OC.Mode(gpu_setup, mode):
        items = OC.draw(OC.pool(K, gpu_setup, mode), 5, 43)
        z = items[0][1]
        canon = items[:2] + [(OC.INF, z, bytes(32), OC.INF)] + items[2:]
        stray = items[:2] + [(OC.INF_STRAY, z, bytes(32), OC.INF_STRAY)] + items[2:]
        r, partial = K.verify_kzg_proof_batch_partial(*OC.columns(canon), gpu_setup)
        assert (r, partial) == K.verify_kzg_proof_batch_partial(*OC.columns(stray), gpu_setup)
        assert r == K.batch_challenge_host(b"".join(b"".join(t) for t in canon), len(canon), mode)
        assert K.verify_kzg_proof_batch(*OC.columns(stray), gpu_setup) is True


def test_empty_batch_null_arguments_and_alignment(K, gpu_setup):
    import torch
    l = K.lib()
    ok = C.c_bool(True)
    buf = _dev(torch, bytes(4 * 160 + 64))
    torch.cuda.synchronize()
    p = buf.data_ptr()
    assert p % 16 == 0
    for mode, empty in ((K.MODE_REFERENCE, False), (K.MODE_CKZG, True), (K.MODE_ETH, True)):
        with OC.Mode(gpu_setup, mode):
            code = OC.mode_code(K, mode)
            assert K.verify_kzg_proof_batch(b"", b"", b"", b"", gpu_setup) is empty
            assert K.verify_kzg_proof_batch_device(None, None, None, None, 0, gpu_setup) is empty
            assert l.lwkzg_verify_kzg_proof_batch(None, b"", b"", b"", b"", 0, gpu_setup.ref()) == K.C_KZG_BADARGS
            assert l.lwkzg_verify_kzg_proof_batch_device(None, p, p, p, p, 1, gpu_setup.ref(), None) == K.C_KZG_BADARGS
            for hole in range(4):
                args = [bytes(48), bytes(32), bytes(32), bytes(48)]
                args[hole] = None
                ok.value = True
                assert l.lwkzg_verify_kzg_proof_batch(C.byref(ok), *args, 1, gpu_setup.ref()) == code
                assert ok.value is False
                ptrs = [p, p + 64, p + 128, p + 192]
                ptrs[hole] = None
                assert l.lwkzg_verify_kzg_proof_batch_device(C.byref(ok), *ptrs, 1, gpu_setup.ref(), None) == code
            # a misaligned device pointer is refused on the host, whichever it is
            for hole in range(4):
                ptrs = [p, p + 64, p + 128, p + 192]
                ptrs[hole] += 8
                assert l.lwkzg_verify_kzg_proof_batch_device(C.byref(ok), *ptrs, 1, gpu_setup.ref(), None) == K.C_KZG_BADARGS
    r, partial = C.create_string_buffer(32), C.create_string_buffer(328)
    assert l.lwkzg_verify_kzg_proof_batch_partial(None, partial, b"", b"", b"", b"", 0, gpu_setup.ref()) == K.C_KZG_BADARGS
    assert l.lwkzg_verify_kzg_proof_batch_partial(r, partial, b"", b"", b"", b"", 0, gpu_setup.ref()) == 0
    assert r.raw == bytes(32) and partial.raw == bytes(328)   # n == 0 writes nothing


def test_inputs_produced_on_the_callers_stream(K, gpu_setup):
    """the four columns are written on a caller stream behind known-long work and verified at once: true; y of one item overwritten on
    the stream: false"""
    import torch
    mode = K.MODE_REFERENCE
    n = 300
    with OC.Mode(gpu_setup, mode):
        items = OC.draw(OC.pool(K, gpu_setup, mode), n, 47)
        cols = OC.columns(items)
        src = [_dev(torch, col) for col in cols]
        dst = [torch.zeros_like(s) for s in src]
        bad_y = _dev(torch, OC.tamper_y(K, mode, items[n - 1])[2])
        filler = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for _ in range(20):
                filler.add_(1.0)
            for d, s in zip(dst, src):
                d.copy_(s, non_blocking=True)
            first = K.verify_kzg_proof_batch_device(*[d.data_ptr() for d in dst], n, gpu_setup, st.cuda_stream)
            for _ in range(20):
                filler.add_(1.0)
            dst[2][32 * (n - 1):32 * n] = bad_y
            second = K.verify_kzg_proof_batch_device(*[d.data_ptr() for d in dst], n, gpu_setup, st.cuda_stream)
            each = K.verify_kzg_proof_each_device(*[d.data_ptr() for d in dst], n, gpu_setup, st.cuda_stream)
        torch.cuda.synchronize()
        assert (first, second) == (True, False)
        assert each == [(0, True)] * (n - 1) + [(0, False)]


def test_second_setup_in_the_same_process(K, gpu_setup):
    """the tau' setup and the tau = 1337 one each verify with their own generator and G2 points"""
    import torch
    n = 5
    other = K.TrustedSetup.from_file(SETUP_TAU2_PATH)
    try:
        blobs = [B.synthetic_blob(59000 + i) for i in range(n)]
        zs = [(1000003 * (i + 2)).to_bytes(32, "big") for i in range(n)]
        mine, theirs = [], []
        for ts, out in ((gpu_setup, mine), (other, theirs)):
            cms = K.blob_to_kzg_commitment_batch(b"".join(blobs), ts)
            res = K.compute_kzg_proof_batch(b"".join(blobs), b"".join(zs), ts)
            out.extend((cms[i], zs[i], res[i][1], res[i][0]) for i in range(n))
        for ts, own, foreign in ((gpu_setup, mine, theirs), (other, theirs, mine)):
            assert _host(K, own, ts) == (0, True, None) and _device(K, torch, own, ts) == (0, True, None)
            assert _host(K, foreign, ts) == (0, False, None) and _device(K, torch, foreign, ts) == (0, False, None)
    finally:
        other.free()


def test_second_truth_known_tau(K, gpu_setup, oracle):
    """reference mode, validly encoded items: the batch is true exactly when the oracle's C - [y]G == [tau - z]pi holds for every item"""
    mode = K.MODE_REFERENCE
    with OC.Mode(gpu_setup, mode):
        honest = OC.draw(OC.pool(K, gpu_setup, mode), 24, 49)
        items, _ = OC.with_defects(K, mode, honest, ["swap_proof", "y_plus_one", "swap_commitment"], 50)
        for batch in (honest, items, items[:12], items[12:]):
            oks = []
            for it in batch:
                rc, ok = oracle.verify_kzg_proof_known_tau(*it, TAU, oracle.MODE_R)
                assert rc == 0
                oks.append(ok)
            assert _host(K, batch, gpu_setup) == (0, all(oks), None)
        assert not all(oracle.verify_kzg_proof_known_tau(*it, TAU, oracle.MODE_R)[1] for it in items)


@pytest.mark.parametrize("n", [1, 65, 1025])
@pytest.mark.parametrize("mode_name", ["reference", "ckzg"])
def test_each_device_equals_the_host_form(K, gpu_setup, mode_name, n):
    import torch
    mode = _mode(K, mode_name)
    with OC.Mode(gpu_setup, mode):
        honest = OC.draw(OC.pool(K, gpu_setup, mode), n, 700 + n)
        items, _ = OC.with_defects(K, mode, honest, OC.VERDICT_KINDS + OC.CODE_KINDS, 800 + n) if n > 1 else ([OC.tamper_y(K, mode, honest[0])], None)
        for batch in (honest, items):
            bufs = [_dev(torch, col) for col in OC.columns(batch)]
            torch.cuda.synchronize()
            got = K.verify_kzg_proof_each_device(*[b.data_ptr() for b in bufs], n, gpu_setup)
            assert got == K.verify_kzg_proof_each(*OC.columns(batch), gpu_setup)
            assert got == OC.truth(K, gpu_setup, mode, batch)
    l = K.lib()
    ok, rc = (C.c_uint8 * 1)(), (C.c_int32 * 1)()
    assert l.lwkzg_verify_kzg_proof_each_device(ok, rc, None, None, None, None, 0, gpu_setup.ref(), None) == 0
    assert l.lwkzg_verify_kzg_proof_each_device(ok, rc, None, None, None, None, 1, gpu_setup.ref(), None) == K.C_KZG_BADARGS
    assert l.lwkzg_verify_kzg_proof_each_device(None, rc, None, None, None, None, 0, gpu_setup.ref(), None) == K.C_KZG_BADARGS
