"""GPU: EIP-7594 cell proof batch verification (lwkzg_verify_cell_kzg_proof_batch, _device, lwkzg_cell_verify_partials) in both modes.
Honest inputs are made on the CPU -- cells by tests/cells_spec.py, proofs and commitments by the closed form over the known tau -- so that
the verifier is not tested only against the library's own generator; r and the four sums of the check are held byte for byte against
the restatement of tests/cell_verify_spec.py on the tau = 1337 and the tau2 setups; every single corruption of one item answers false;
malformed inputs give the mode's code; the forms, engines and modes agree; and a batch of 72 blobs x 128 cells made by
compute_cells_and_kzg_proofs_batch crosses the launch-set boundaries of the engine and of vmsm.hip."""
import contextlib
import ctypes as C
import random

import pytest

import blobs as B
import cell_verify_spec as V
import cells_spec as S
import make_setups as M
from conftest import P, R, SETUP_PATH, SETUP_TAU2_PATH, TAU, tau_closed_form

pytestmark = pytest.mark.gpu

INF = bytes([0xc0]) + bytes(47)
MODES = [S.MODE_REFERENCE, S.MODE_CKZG]


@contextlib.contextmanager
def _mode(K, ts, mode):
    K.lib().lwkzg_settings_set_mode(ts.ref(), mode)
    try:
        yield
    finally:
        K.lib().lwkzg_settings_set_mode(ts.ref(), -1)


class Poly:
    """a polynomial with its commitment, cell values and (lazily) cell proofs, all computed on the CPU for a known tau"""
    _cache = {}

    def __init__(self, oracle, coeffs, tau):
        self.oracle, self.p, self.tau = oracle, coeffs, tau
        self.cm = tau_closed_form(oracle, coeffs, tau=tau)
        self.values = S.cell_values(coeffs)
        self.proofs = {}

    @classmethod
    def seeded(cls, oracle, seed, tau=TAU):
        if (seed, tau) not in cls._cache:
            rnd = random.Random(seed)
            cls._cache[(seed, tau)] = cls(oracle, [rnd.randrange(R) for _ in range(S.N_BLOB)], tau)
        return cls._cache[(seed, tau)]

    def cell(self, k, mode):
        return b"".join(S.to_bytes(v, mode) for v in self.values[64 * k:64 * k + 64])

    def proof(self, k):
        if k not in self.proofs:
            self.proofs[k] = tau_closed_form(self.oracle, S.quotient(self.p, k), tau=self.tau)
        return self.proofs[k]

    def item(self, k, mode):
        return (self.cm, k, self.cell(k, mode), self.proof(k))


def _verify(K, ts, items):
    return K.verify_cell_kzg_proof_batch([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items], ts)


def _partials(K, ts, items):
    return K.cell_verify_partials([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items], ts)


def _rc(K, ts, items):
    ok = C.c_bool(True)
    idx = (C.c_uint64 * max(len(items), 1))(*[i[1] for i in items])
    rc = K.lib().lwkzg_verify_cell_kzg_proof_batch(C.byref(ok), b"".join(i[0] for i in items), idx, b"".join(i[2] for i in items),
                                                   b"".join(i[3] for i in items), len(items), ts.ref())
    return rc, bool(ok.value)


def _device(K, ts, items, stream=None):
    import torch

    def dev(data):
        return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()

    dc, dcell, dp = dev(b"".join(i[0] for i in items)), dev(b"".join(i[2] for i in items)), dev(b"".join(i[3] for i in items))
    di = torch.tensor([i[1] for i in items] or [0], dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    return K.verify_cell_kzg_proof_batch_device(dc.data_ptr(), di.data_ptr(), dcell.data_ptr(), dp.data_ptr(), len(items), ts, stream)


def _sidecar(oracle, mode, tau=TAU, blobs=16, base=3000):
    """one column of `blobs` blobs and four columns of half of them"""
    polys = [Poly.seeded(oracle, base + j, tau) for j in range(blobs)]
    items = [p.item(5, mode) for p in polys]
    for k in (10, 64, 100, 127):
        items += [p.item(k, mode) for p in polys[:blobs // 2]]
    return items


def _honest_batches(oracle, mode):
    two = [Poly.seeded(oracle, 3100 + j) for j in range(2)]
    sidecar = _sidecar(oracle, mode)
    shuffled = list(sidecar)
    random.Random(7).shuffle(shuffled)
    few = [Poly.seeded(oracle, 3000 + j).item(k, mode) for j, k in [(0, 5), (1, 5), (0, 10)]]
    return {
        "all_cells_of_two_blobs": [p.item(k, mode) for p in two for k in range(128)],
        "column_sidecars": sidecar,
        "shuffled": shuffled,
        "repeated_item": few + [few[1], few[0], few[1]],
    }


@pytest.mark.parametrize("mode", MODES)
def test_honest_batches_answer_true_and_their_sums_are_the_restatement(K, gpu_setup, oracle, mode):
    for name, items in _honest_batches(oracle, mode).items():
        with _mode(K, gpu_setup, mode):
            assert _verify(K, gpu_setup, items) is True, name
            got = _partials(K, gpu_setup, items)
        assert got == V.partials_bytes(oracle, items, mode, TAU), name


@pytest.mark.parametrize("mode", MODES)
def test_sums_on_the_second_setup(K, oracle, mode):
    items = _sidecar(oracle, mode, tau=M.TAU2, blobs=4, base=3200)
    ts = K.TrustedSetup.from_file(SETUP_TAU2_PATH)
    try:
        with _mode(K, ts, mode):
            assert _verify(K, ts, items) is True
            assert _partials(K, ts, items) == V.partials_bytes(oracle, items, mode, M.TAU2)
    finally:
        ts.free()


def _small_batch(oracle, mode):
    polys = [Poly.seeded(oracle, 3000 + j) for j in range(3)]
    return [p.item(k, mode) for k in (5, 10, 64, 127) for p in polys], polys


def _corruptions(item, polys, mode):
    c, k, cell, proof = item
    owner = next(p for p in polys if p.cm == c)
    other = next(p for p in polys if p.cm != c)
    t = 33
    v = (S.element(cell[32 * t:32 * t + 32], mode) + 1) % R
    return {
        "cell_element": (c, k, cell[:32 * t] + S.to_bytes(v, mode) + cell[32 * t + 32:], proof),
        "neighbours_proof": (c, k, cell, owner.proof(k ^ 1)),
        "another_blobs_commitment": (other.cm, k, cell, proof),
        "another_column": (c, 10 if k != 10 else 64, cell, proof),
    }


@pytest.mark.parametrize("mode", MODES)
def test_every_single_corruption_answers_false(K, gpu_setup, oracle, mode):
    items, polys = _small_batch(oracle, mode)
    with _mode(K, gpu_setup, mode):
        assert _rc(K, gpu_setup, items) == (K.C_KZG_OK, True)
        for pos in (0, len(items) // 2, len(items) - 1):
            for name, bad in _corruptions(items[pos], polys, mode).items():
                batch = items[:pos] + [bad] + items[pos + 1:]
                assert _rc(K, gpu_setup, batch) == (K.C_KZG_OK, False), (pos, name)


def _x_off_the_curve():
    for x in range(1, 100):
        if pow(x ** 3 + 4, (P - 1) // 2, P) != 1:
            b = bytearray(x.to_bytes(48, "big"))
            b[0] |= 0x80
            return bytes(b)


@pytest.mark.parametrize("mode", MODES)
def test_malformed_inputs_give_the_modes_code(K, gpu_setup, oracle, mode):
    items, _ = _small_batch(oracle, mode)
    want = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    order3 = bytes([0x80]) + bytes(47)            # (0, 2): on the curve, of order 3
    assert oracle.g1_decompress(order3) is None and oracle.g1_decompress(_x_off_the_curve()) is None
    c, k, cell, proof = items[4]
    with _mode(K, gpu_setup, mode):
        for name, bad in [("proof outside the subgroup", (c, k, cell, order3)), ("proof off the curve", (c, k, cell, _x_off_the_curve())),
                          ("commitment outside the subgroup", (order3, k, cell, proof)),
                          ("element equal to r", (c, k, cell[:64] + S.to_bytes(R, mode) + cell[96:], proof)),
                          ("element 2^256 - 1", (c, k, cell[:2016] + b"\xff" * 32, proof))]:
            for pos in (0, 4, len(items) - 1):
                batch = items[:pos] + [bad] + items[pos + 1:]
                assert _rc(K, gpu_setup, batch) == (want, False), (name, pos)
        # r - 1 is a value like any other: the call answers, and the answer is false
        assert _rc(K, gpu_setup, items[:4] + [(c, k, cell[:64] + S.to_bytes(R - 1, mode) + cell[96:], proof)] + items[5:]) == (K.C_KZG_OK, False)
        assert _rc(K, gpu_setup, items[:4] + [(c, 128, cell, proof)] + items[5:]) == (K.C_KZG_BADARGS, False)
        assert _rc(K, gpu_setup, items) == (K.C_KZG_OK, True)      # and the settings object is none the worse


@pytest.mark.parametrize("mode", MODES)
def test_small_and_degenerate_batches(K, gpu_setup, oracle, mode):
    gen12345 = oracle.g1_generator_mul(12345)
    with _mode(K, gpu_setup, mode):
        assert _rc(K, gpu_setup, []) == (K.C_KZG_OK, True)
        assert _device(K, gpu_setup, []) is True
        one = Poly.seeded(oracle, 3000).item(77, mode)
        assert _verify(K, gpu_setup, [one]) is True
        assert _verify(K, gpu_setup, [(one[0], 78, one[2], one[3])]) is False
        # the zero blob: C = pi = infinity, every cell zero
        zero = [(INF, k, bytes(2048), INF) for k in (0, 64, 127)]
        assert _verify(K, gpu_setup, zero) is True
        assert _partials(K, gpu_setup, zero)[32:] == (b"\x01" + bytes(96)) * 4
        assert _verify(K, gpu_setup, zero + [(INF, 3, bytes(2016) + S.to_bytes(1, mode), INF)]) is False
        # a constant polynomial: every proof is infinity, the commitment is not
        const = [(gen12345, k, S.to_bytes(12345, mode) * 64, INF) for k in (1, 2, 100)]
        assert _verify(K, gpu_setup, const) is True
        assert _verify(K, gpu_setup, const + zero + [one]) is True
        assert _verify(K, gpu_setup, const + [(gen12345, 9, S.to_bytes(12346, mode) * 64, INF)]) is False


@pytest.mark.parametrize("mode", MODES)
def test_host_and_device_forms_streams_and_repeats_agree(K, gpu_setup, oracle, mode):
    import torch
    items = _sidecar(oracle, mode)
    bad = list(items)
    bad[20] = (bad[20][0], bad[20][1], bad[20][2], bad[21][3])
    with _mode(K, gpu_setup, mode):
        first = _partials(K, gpu_setup, items)
        for batch, want in [(items, True), (bad, False)]:
            assert _verify(K, gpu_setup, batch) is want
            assert _device(K, gpu_setup, batch) is want
            assert _verify(K, gpu_setup, batch) is want       # a second call with the same inputs
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                assert _device(K, gpu_setup, batch, s.cuda_stream) is want
            s.synchronize()
        assert _partials(K, gpu_setup, items) == first


@pytest.mark.parametrize("mode", MODES)
def test_both_engines(K, engine_setup, oracle, mode):
    items = _sidecar(oracle, mode)
    with _mode(K, engine_setup, mode):
        assert _verify(K, engine_setup, items) is True
        assert _partials(K, engine_setup, items) == V.partials_bytes(oracle, items, mode, TAU)
        assert _verify(K, engine_setup, items[:-1] + [items[-1][:3] + (items[0][3],)]) is False


def test_lagrange_only_table_in_ckzg_mode(K, oracle):
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        ts.set_mode(K.MODE_CKZG)
        ts.enable_direct_table_forms(10, 2)
        assert ts.direct_table_forms() == 2
        items = _sidecar(oracle, S.MODE_CKZG)
        assert _verify(K, ts, items) is True
        assert _partials(K, ts, items) == V.partials_bytes(oracle, items, S.MODE_CKZG, TAU)
        assert _verify(K, ts, items[1:] + [items[0][:2] + (items[1][2], items[0][3])]) is False
    finally:
        ts.free()


def test_reference_mode_and_ckzg_mode_agree_on_the_same_polynomial(K, gpu_setup, oracle):
    verdicts, sums = {}, {}
    for mode in MODES:
        items = _sidecar(oracle, mode)
        assert [i[0] for i in items] == [i[0] for i in _sidecar(oracle, 1 - mode)]        # same commitments and proofs,
        assert items[0][2] == b"".join(_sidecar(oracle, 1 - mode)[0][2][32 * t:32 * t + 32][::-1] for t in range(64))   # cells byte-reversed
        with _mode(K, gpu_setup, mode):
            verdicts[mode] = (_verify(K, gpu_setup, items), _verify(K, gpu_setup, items[:5] + [items[5][:3] + (INF,)] + items[6:]))
    assert verdicts[S.MODE_REFERENCE] == verdicts[S.MODE_CKZG] == (True, False)


@pytest.mark.parametrize("mode", MODES)
def test_large_batch_made_by_the_library(K, gpu_setup, mode):
    n_blobs = 72
    blobs = b"".join(B.synthetic_blob(900 + i, big_endian=mode == S.MODE_REFERENCE) for i in range(n_blobs))
    with _mode(K, gpu_setup, mode):
        comms = K.blob_to_kzg_commitment_batch(blobs, gpu_setup)
        made = K.compute_cells_and_kzg_proofs_batch(blobs, gpu_setup)
        cm = b"".join(c * 128 for c in comms)
        idx = list(range(128)) * n_blobs
        cells = b"".join(b"".join(c) for c, _ in made)
        proofs = b"".join(b"".join(p) for _, p in made)
        assert K.verify_cell_kzg_proof_batch(cm, idx, cells, proofs, gpu_setup) is True
        at = (40 * 128 + 93) * 2048 + 32 * 21 + (31 if mode == S.MODE_REFERENCE else 0)   # the low byte of an element
        flipped = cells[:at] + bytes([cells[at] ^ 1]) + cells[at + 1:]
        assert K.verify_cell_kzg_proof_batch(cm, idx, flipped, proofs, gpu_setup) is False
        # the last item's proof swapped for the first one's: the last slice of the variable-base sums
        assert K.verify_cell_kzg_proof_batch(cm, idx, cells, proofs[:-48] + proofs[:48], gpu_setup) is False


def _g2_lines(path):
    lines = open(path).read().split()
    n1, n2 = int(lines[0]), int(lines[1])
    return [bytes.fromhex(x) for x in lines[2 + n1:2 + n1 + n2]]


@pytest.mark.parametrize("mode", MODES)
def test_verdict_equals_the_host_pairing_on_the_per_item_equation(K, gpu_setup, oracle, mode):
    g2 = _g2_lines(SETUP_PATH)
    poly = Poly.seeded(oracle, 3000)
    p_tau = S.evaluate(poly.p, TAU)
    honest = poly.item(77, mode)
    cases = [honest, honest[:3] + (poly.proof(78),), (honest[0], 77, poly.cell(76, mode), honest[3])]
    verdicts = []
    for c, k, cell, proof in cases:
        i_tau = S.evaluate(V.interpolant_by_transform(V.cell_elements(cell, mode), k), TAU)
        lhs_g2 = M.g2_compress(M.g2_mul_generator((pow(TAU, 64, R) - S.c_of_cell(k)) % R))
        i_g1 = oracle.g1_generator_mul((i_tau - p_tau) % R)
        want = K.capi.pairing_product_is_one(proof + i_g1, lhs_g2 + g2[0])
        with _mode(K, gpu_setup, mode):
            assert _verify(K, gpu_setup, [(c, k, cell, proof)]) is want
        assert V.item_holds_known_tau(oracle, (c, k, cell, proof), mode, TAU) is want
        verdicts.append(want)
    assert verdicts == [True, False, False]
