"""GPU: cell proof verification of whole blobs (lwkzg_verify_blob_cell_kzg_proofs_batch / _groups, their device forms and partials
hooks). The calls are defined by the calls over items, so the checks are equalities: the partials of a call over
blobs are, byte for byte, those of the existing call over the 128 n expanded items (cells from the library's compute call), in all
three modes, on the bucket engine and on a direct table, and the device forms answer what the host forms answer. Beside that: an
honest polynomial that the library did not make (commitment and proofs by the closed form over the known tau); every single
corruption; malformed inputs; groups, where a bad or rejected blob changes exactly its own group; the chunk boundary of the
extension on the device; and no allocation in steady state."""
import contextlib
import ctypes as C

import pytest

import blobs as B
import cells_spec as S
from conftest import R, SETUP_PATH
from test_gpu_cell_verify import Poly

pytestmark = pytest.mark.gpu

MODE_ETH = 2
MODES = [S.MODE_REFERENCE, S.MODE_CKZG, MODE_ETH]
INF = bytes([0xc0]) + bytes(47)
ORDER3 = bytes([0x80]) + bytes(47)     # (0, 2): on the curve, of order 3
BLOB_BYTES, CELLS, CELLS_CHUNK = 4096 * 32, 128, 512   # cells_common.h: kCellsChunk


@contextlib.contextmanager
def _mode(K, ts, mode):
    K.lib().lwkzg_settings_set_mode(ts.ref(), mode)
    try:
        yield
    finally:
        K.lib().lwkzg_settings_set_mode(ts.ref(), -1)


def _el(x, mode):
    return x.to_bytes(32, "little" if mode == S.MODE_CKZG else "big")


def _bad_code(K, mode):
    return K.C_KZG_ERROR if mode == S.MODE_REFERENCE else K.C_KZG_BADARGS


class Made:
    """six distinct blobs in `mode`'s bytes with what the library's own calls give for them: computed once per mode, never changed"""
    _cache = {}

    def __init__(self, K, ts, mode):
        self.mode = mode
        self.blobs = [B.synthetic_blob(700 + i, big_endian=mode != S.MODE_CKZG) for i in range(6)]
        with _mode(K, ts, mode):
            self.comms = K.blob_to_kzg_commitment_batch(b"".join(self.blobs), ts)
            made = K.compute_cells_and_kzg_proofs_batch(b"".join(self.blobs), ts)
        self.cells = [b"".join(c) for c, _ in made]
        self.proofs = [b"".join(p) for _, p in made]

    @classmethod
    def of(cls, K, ts, mode):
        if mode not in cls._cache:
            cls._cache[mode] = cls(K, ts, mode)
        return cls._cache[mode]

    def call(self, order):
        """(blobs, commitments, cell proofs) of the blobs `order` names"""
        return [self.blobs[j] for j in order], [self.comms[j] for j in order], [self.proofs[j] for j in order]

    def expanded(self, blobs, comms, proofs):
        """the four item arrays of the existing calls for a call over blobs (each blob one of the six, possibly with other proofs)"""
        cells = b"".join(self.cells[self.blobs.index(b)] for b in blobs)
        return b"".join(c * CELLS for c in comms), list(range(CELLS)) * len(blobs), cells, b"".join(proofs)


def _items(cm, idx, cells, proofs, lo, hi):
    return [(cm[48 * i:48 * i + 48], idx[i], cells[2048 * i:2048 * i + 2048], proofs[48 * i:48 * i + 48]) for i in range(lo, hi)]


def _rc(K, ts, blobs, comms, proofs):
    ok = C.c_bool(True)
    rc = K.lib().lwkzg_verify_blob_cell_kzg_proofs_batch(C.byref(ok), b"".join(blobs), b"".join(comms), b"".join(proofs), len(blobs), ts.ref())
    return rc, bool(ok.value)


def _dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _rc_device(K, ts, blobs, comms, proofs, stream=None):
    import torch
    db, dc, dp = _dev(b"".join(blobs)), _dev(b"".join(comms)), _dev(b"".join(proofs))
    torch.cuda.synchronize()
    ok = C.c_bool(True)
    rc = K.lib().lwkzg_verify_blob_cell_kzg_proofs_batch_device(C.byref(ok), db.data_ptr(), dc.data_ptr(), dp.data_ptr(), len(blobs), ts.ref(),
                                                                stream)
    return rc, bool(ok.value)


def _groups_device(K, ts, blobs, comms, proofs, sizes):
    import torch
    db, dc, dp = _dev(b"".join(blobs)), _dev(b"".join(comms)), _dev(b"".join(proofs))
    torch.cuda.synchronize()
    return K.verify_blob_cell_kzg_proofs_groups_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), len(blobs), sizes, ts)


# ---- honest inputs that the library did not make ----------------------------------------------------------------------------------------
def _blob_of(p, mode):
    if mode == S.MODE_REFERENCE:
        return S.blob_from_poly(p, mode)
    return b"".join(_el(v, mode) for v in S.brp(S.ntt(list(p), S.W4096)))


@pytest.mark.parametrize("mode", MODES)
def test_an_honest_polynomial_over_the_known_tau_answers_true(K, gpu_setup, oracle, mode):
    poly = Poly.seeded(oracle, 3100)
    blob, proofs = _blob_of(poly.p, mode), [b"".join(poly.proof(k) for k in range(CELLS))]
    with _mode(K, gpu_setup, mode):
        assert _rc(K, gpu_setup, [blob], [poly.cm], proofs) == (K.C_KZG_OK, True)
        assert _rc_device(K, gpu_setup, [blob], [poly.cm], proofs) == (K.C_KZG_OK, True)
        assert K.verify_blob_cell_kzg_proofs_groups(blob, poly.cm, proofs[0], [1], gpu_setup) == [(K.C_KZG_OK, True)]
        swapped = proofs[0][48:96] + proofs[0][:48] + proofs[0][96:]
        assert _rc(K, gpu_setup, [blob], [poly.cm], [swapped]) == (K.C_KZG_OK, False)


# ---- equality with the existing calls, byte for byte ---------------------------------------------------------------------------------------
SHAPES = {"one": ([0], [1]), "same_blob_twice": ([0, 0], [2]), "A_B_A": ([0, 1, 0], [2, 1]),
          "sixty_five": ([j % 3 for j in range(65)], [1, 0, 64])}     # 65 blobs cross kHostSlice in the host forms


def _check_equal_to_the_item_calls(K, ts, made, order, sizes):
    blobs, comms, proofs = made.call(order)
    cm, idx, cells, pf = made.expanded(blobs, comms, proofs)
    want = K.cell_verify_partials(cm, idx, cells, pf, ts)
    assert K.blob_cell_verify_partials(blobs, comms, proofs, ts) == want
    assert _rc(K, ts, blobs, comms, proofs) == (K.C_KZG_OK, True) == _rc_device(K, ts, blobs, comms, proofs)
    groups, lo = [], 0
    for m in sizes:
        groups.append(_items(cm, idx, cells, pf, CELLS * lo, CELLS * (lo + m)))
        lo += m
    want_g = K.cell_verify_groups_partials(groups, ts)
    assert K.blob_cell_verify_groups_partials(blobs, comms, proofs, sizes, ts) == want_g
    answers = K.verify_blob_cell_kzg_proofs_groups(blobs, comms, proofs, sizes, ts)
    assert answers == [(K.C_KZG_OK, True)] * len(sizes) == K.verify_cell_kzg_proof_groups(groups, ts)
    assert _groups_device(K, ts, blobs, comms, proofs, sizes) == answers
    if len(sizes) == 1:
        assert want_g[0] == want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ["one", "same_blob_twice", "A_B_A"])
def test_partials_equal_those_of_the_calls_over_the_expanded_items(K, gpu_setup, mode, shape):
    made = Made.of(K, gpu_setup, mode)
    with _mode(K, gpu_setup, mode):
        _check_equal_to_the_item_calls(K, gpu_setup, made, *SHAPES[shape])


def test_sixty_five_blobs_cross_the_host_slice(K, gpu_setup):
    made = Made.of(K, gpu_setup, MODE_ETH)
    with _mode(K, gpu_setup, MODE_ETH):
        _check_equal_to_the_item_calls(K, gpu_setup, made, *SHAPES["sixty_five"])


@pytest.fixture(scope="module")
def direct10_setup(K):
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    ts.enable_direct_table(10)
    assert ts.direct_table_bits() == 10
    yield ts
    ts.free()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("engine", ["bucket", "direct10"])
def test_equality_on_the_bucket_engine_and_on_a_direct_table(K, gpu_setup, bucket_setup, direct10_setup, mode, engine):
    made = Made.of(K, gpu_setup, mode)
    ts = bucket_setup if engine == "bucket" else direct10_setup
    with _mode(K, ts, mode):
        _check_equal_to_the_item_calls(K, ts, made, *SHAPES["A_B_A"])


# ---- every single corruption answers false -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_single_corruption_answers_false(K, gpu_setup, mode):
    made = Made.of(K, gpu_setup, mode)
    blobs, comms, proofs = made.call([0, 1, 2])
    low = 0 if mode == S.MODE_CKZG else 31       # the low byte of an element: the elements stay below 2^248
    with _mode(K, gpu_setup, mode):
        assert _rc(K, gpu_setup, blobs, comms, proofs) == (K.C_KZG_OK, True)
        for b in (0, 2):
            other = made.proofs[1]
            for k in (0, 63, 64, 127):
                pf = proofs[b]
                theirs = proofs[:b] + [pf[:48 * k] + other[48 * k:48 * k + 48] + pf[48 * k + 48:]] + proofs[b + 1:]
                assert _rc(K, gpu_setup, blobs, comms, theirs) == (K.C_KZG_OK, False), ("another blob's proof", b, k)
                k2 = (k + 65) % CELLS
                sw = bytearray(pf)
                sw[48 * k:48 * k + 48], sw[48 * k2:48 * k2 + 48] = pf[48 * k2:48 * k2 + 48], pf[48 * k:48 * k + 48]
                assert _rc(K, gpu_setup, blobs, comms, proofs[:b] + [bytes(sw)] + proofs[b + 1:]) == (K.C_KZG_OK, False), ("swapped", b, k, k2)
            at = 32 * 1234 + low
            changed = blobs[b][:at] + bytes([blobs[b][at] ^ 1]) + blobs[b][at + 1:]
            assert _rc(K, gpu_setup, blobs[:b] + [changed] + blobs[b + 1:], comms, proofs) == (K.C_KZG_OK, False), ("a blob byte", b)
            assert _rc(K, gpu_setup, blobs, comms[:b] + [made.comms[3]] + comms[b + 1:], proofs) == (K.C_KZG_OK, False), ("commitment", b)
        assert _rc_device(K, gpu_setup, blobs, comms, proofs[:2] + [proofs[2][:-48] + proofs[0][:48]]) == (K.C_KZG_OK, False)
        assert _rc(K, gpu_setup, blobs, comms, proofs) == (K.C_KZG_OK, True)


# ---- malformed inputs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_malformed_inputs_give_the_modes_code(K, gpu_setup, mode):
    made = Made.of(K, gpu_setup, mode)
    blobs, comms, proofs = made.call([0, 1, 2])
    want = (_bad_code(K, mode), False)
    t = 4095
    equal_r = blobs[2][:32 * t] + _el(R, mode) + blobs[2][32 * t + 32:]
    with _mode(K, gpu_setup, mode):
        for name, call in [("a proof outside G1", (blobs, comms, proofs[:1] + [proofs[1][:48 * 64] + ORDER3 + proofs[1][48 * 65:]] + proofs[2:])),
                           ("a commitment outside G1", (blobs, [comms[0], ORDER3, comms[2]], proofs))]:
            assert _rc(K, gpu_setup, *call) == want, name
            assert _rc_device(K, gpu_setup, *call) == want, name
        rejected = (blobs[:2] + [equal_r], comms, proofs)
        if mode == S.MODE_REFERENCE:
            # reference mode reduces: r stands for 0, which is another polynomial; e + r stands for e, which is the same one
            assert _rc(K, gpu_setup, *rejected) == (K.C_KZG_OK, False)
            e = int.from_bytes(blobs[2][32 * t:32 * t + 32], "big")
            same = blobs[2][:32 * t] + _el(e + R, mode) + blobs[2][32 * t + 32:]
            assert _rc(K, gpu_setup, blobs[:2] + [same], comms, proofs) == (K.C_KZG_OK, True)
        else:
            assert _rc(K, gpu_setup, *rejected) == want
            assert _rc_device(K, gpu_setup, *rejected) == want
        # the zero blob: its commitment and all its proofs are the infinity encoding, accepted as the batch call accepts it
        zero = ([bytes(BLOB_BYTES)], [INF], [INF * CELLS])
        assert _rc(K, gpu_setup, *zero) == (K.C_KZG_OK, True)
        assert _rc(K, gpu_setup, blobs[:1] + zero[0], comms[:1] + zero[1], proofs[:1] + zero[2]) == (K.C_KZG_OK, True)
        assert _rc(K, gpu_setup, zero[0], [INF], [INF * 127 + proofs[0][:48]]) == (K.C_KZG_OK, False)
        assert _rc(K, gpu_setup, blobs, comms, proofs) == (K.C_KZG_OK, True)      # and the settings object is none the worse


# ---- groups --------------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 0, 2, 3]     # offsets [0, 1, 1, 3, 6]: a one-blob transaction, an empty group, a two-blob and a three-blob one


@pytest.mark.parametrize("mode", MODES)
def test_groups_a_bad_blob_changes_exactly_its_group(K, gpu_setup, mode):
    made = Made.of(K, gpu_setup, mode)
    blobs, comms, proofs = made.call(range(6))
    good = (K.C_KZG_OK, True)
    with _mode(K, gpu_setup, mode):
        honest = K.verify_blob_cell_kzg_proofs_groups(blobs, comms, proofs, SIZES, gpu_setup)
        assert honest == [good] * 4
        parts = K.blob_cell_verify_groups_partials(blobs, comms, proofs, SIZES, gpu_setup)
        assert parts[1] == bytes(len(parts[1]))
        assert K.verify_blob_cell_kzg_proofs_groups(blobs, comms, proofs, [6], gpu_setup) == [_rc(K, gpu_setup, blobs, comms, proofs)] == [good]
        # one proof of blob 4 (group 3) is blob 3's
        bad_pf = proofs[:4] + [proofs[4][:48 * 127] + proofs[3][48 * 127:]] + proofs[5:]
        assert K.verify_blob_cell_kzg_proofs_groups(blobs, comms, bad_pf, SIZES, gpu_setup) == [good, good, good, (K.C_KZG_OK, False)]
        assert _groups_device(K, gpu_setup, blobs, comms, bad_pf, SIZES) == [good, good, good, (K.C_KZG_OK, False)]
        got = K.blob_cell_verify_groups_partials(blobs, comms, bad_pf, SIZES, gpu_setup)
        assert got[:3] == parts[:3] and got[3] != parts[3]
        assert K.verify_blob_cell_kzg_proofs_groups(blobs, comms, bad_pf, [6], gpu_setup) == [_rc(K, gpu_setup, blobs, comms, bad_pf)] == [(K.C_KZG_OK, False)]
        # an element of blob 2 (group 2) equal to r
        bad_blobs = blobs[:2] + [blobs[2][:32 * 77] + _el(R, mode) + blobs[2][32 * 78:]] + blobs[3:]
        answer = (K.C_KZG_OK, False) if mode == S.MODE_REFERENCE else (_bad_code(K, mode), False)
        assert K.verify_blob_cell_kzg_proofs_groups(bad_blobs, comms, proofs, SIZES, gpu_setup) == [good, good, answer, good]
        assert _groups_device(K, gpu_setup, bad_blobs, comms, proofs, SIZES) == [good, good, answer, good]
        got = K.blob_cell_verify_groups_partials(bad_blobs, comms, proofs, SIZES, gpu_setup)
        assert got[:2] == parts[:2] and got[3] == parts[3]
        if mode != S.MODE_REFERENCE:
            assert got[2] == bytes(len(got[2]))      # nothing behind r ran on the group
        assert K.verify_blob_cell_kzg_proofs_groups(bad_blobs, comms, proofs, [6], gpu_setup) == [_rc(K, gpu_setup, bad_blobs, comms, proofs)] == [answer]


# ---- the chunk boundary of the extension, on the device ------------------------------------------------------------------------------------
def test_one_blob_more_than_a_chunk_on_the_device(K, gpu_setup):
    import torch
    n = CELLS_CHUNK + 1
    made = Made.of(K, gpu_setup, S.MODE_CKZG)
    three = _dev(b"".join(made.blobs[:3])).view(3, BLOB_BYTES)
    comms3 = _dev(b"".join(made.comms[:3])).view(3, 48)
    proofs3 = torch.empty((3, CELLS * 48), dtype=torch.uint8, device="cuda")
    pick = torch.arange(n, device="cuda") % 3
    with _mode(K, gpu_setup, S.MODE_CKZG):
        torch.cuda.synchronize()
        K.compute_cells_and_kzg_proofs_batch_device(None, proofs3.data_ptr(), three.data_ptr(), 3, gpu_setup)
        torch.cuda.synchronize()
        blobs, comms, proofs = three[pick].contiguous(), comms3[pick].contiguous(), proofs3[pick].contiguous()
        torch.cuda.synchronize()
        args = (blobs.data_ptr(), comms.data_ptr(), proofs.data_ptr(), n, gpu_setup)
        assert K.verify_blob_cell_kzg_proofs_batch_device(*args) is True
        proofs[n - 1, 48 * 5:48 * 6] = proofs[n - 1, 48 * 6:48 * 7].clone()     # one proof of the last blob overwritten
        torch.cuda.synchronize()
        assert K.verify_blob_cell_kzg_proofs_batch_device(*args) is False


# ---- no allocation in steady state ---------------------------------------------------------------------------------------------------------
def test_a_second_call_of_the_same_shape_allocates_nothing(K, gpu_setup):
    import torch
    made = Made.of(K, gpu_setup, MODE_ETH)
    blobs, comms, proofs = made.call([0, 1, 0, 2, 3])
    db, dc, dp = _dev(b"".join(blobs)), _dev(b"".join(comms)), _dev(b"".join(proofs))
    calls = [lambda: K.verify_blob_cell_kzg_proofs_batch(blobs, comms, proofs, gpu_setup),
             lambda: K.verify_blob_cell_kzg_proofs_batch_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), 5, gpu_setup),
             lambda: K.verify_blob_cell_kzg_proofs_groups(blobs, comms, proofs, [2, 0, 3], gpu_setup),
             lambda: K.verify_blob_cell_kzg_proofs_groups_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), 5, [2, 0, 3], gpu_setup)]
    with _mode(K, gpu_setup, MODE_ETH):
        for call in calls:
            first = call()
            torch.cuda.synchronize()
            free = torch.cuda.mem_get_info()[0]      # hipMemGetInfo
            assert call() == first
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free
