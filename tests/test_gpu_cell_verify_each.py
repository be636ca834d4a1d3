"""GPU: per-item EIP-7594 cell proof verification (lwkzg_verify_cell_kzg_proof_each, _device, lwkzg_cell_verify_each_points) in both
modes. Honest items are made on the CPU as tests/test_gpu_cell_verify.py makes them (cells by tests/cells_spec.py, commitments and
proofs by the closed form over the known tau). Every verdict is held against the check done in G1 with tau known; every (rc, ok)
against lwkzg_verify_cell_kzg_proof_batch on the item alone; the point each pairing is taken of, byte for byte, against the restatement
of tests/cell_verify_spec.py on both setups; polynomials of degree < 64 drive the reduction tree of k_celleach_commit through equal,
opposite and absent partial points; and the shapes cross the 64-lane blocks and the capacity steps of the context's buffer."""
import pytest

import cell_verify_spec as V
import cells_spec as S
import make_setups as M
from conftest import R, SETUP_TAU2_PATH, TAU
from test_gpu_cell_verify import INF, MODES, Poly, _corruptions, _mode, _rc, _x_off_the_curve

pytestmark = pytest.mark.gpu

ORDER3 = bytes([0x80]) + bytes(47)            # (0, 2): on the curve, of order 3


def _each(K, ts, items):
    return K.verify_cell_kzg_proof_each([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items], ts)


def _points(K, ts, items):
    return K.cell_verify_each_points([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items], ts)


def _device(K, ts, items, stream=None):
    """the device form; with a stream, the inputs are produced on it and nothing waits for them before the call"""
    import torch

    def dev(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(non_blocking=True)

    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        dc, dcell, dp = dev(b"".join(i[0] for i in items)), dev(b"".join(i[2] for i in items)), dev(b"".join(i[3] for i in items))
        di = torch.tensor([i[1] for i in items], dtype=torch.int64).cuda(non_blocking=True)
    if stream is None:
        torch.cuda.synchronize()
    got = K.verify_cell_kzg_proof_each_device(dc.data_ptr(), di.data_ptr(), dcell.data_ptr(), dp.data_ptr(), len(items), ts,
                                              None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    return got


def _want_point(oracle, item, mode, tau):
    """P = RLC - RLI + RLP of the item alone (r^0 = 1), in the hook's layout"""
    _, _, rlc, rli, rlp = V.sums(oracle, [item], mode, tau)
    xy, inf = V._add(oracle, V._add(oracle, rlc, V._neg(rli)), rlp)
    return (b"\x01" + bytes(96)) if inf else (b"\x00" + xy)


def _polys(oracle):
    return [Poly.seeded(oracle, 3000 + j) for j in range(3)]


def _honest(oracle, mode):
    return [p.item(k, mode) for k in (5, 10, 64, 127) for p in _polys(oracle)]


@pytest.fixture(scope="module")
def tau2_setup(K):
    ts = K.TrustedSetup.from_file(SETUP_TAU2_PATH)
    yield ts
    ts.free()


@pytest.mark.parametrize("mode", MODES)
def test_verdicts_against_independent_truth(K, gpu_setup, oracle, mode):
    items, polys = _honest(oracle, mode), _polys(oracle)
    batch = list(items)
    for pos in (0, 5, len(items) - 1):
        c, k, cell, proof = items[pos]
        batch += list(_corruptions(items[pos], polys, mode).values())       # one element, a neighbour's proof, another commitment, another index
        batch.append((c, k, cell, oracle.g1_generator_mul(99 + pos)))        # a proof of nothing
        batch.append(items[(pos + 1) % len(items)])                          # honest items between the bad ones
    want = [V.item_holds_known_tau(oracle, it, mode, TAU) for it in batch]
    assert want[:len(items)] == [True] * len(items) and want.count(False) == 15
    with _mode(K, gpu_setup, mode):
        got = _each(K, gpu_setup, batch)
    assert [rc for rc, _ in got] == [K.C_KZG_OK] * len(batch)
    assert [ok for _, ok in got] == want


def _mixed_batch(oracle, mode):
    """(items, the positions of the good ones): every kind of bad item with a good neighbour on both sides"""
    good = _honest(oracle, mode)
    c, k, cell, proof = good[4]
    top = 31 if mode == S.MODE_CKZG else 0                               # the most significant byte in the mode's order
    only_here = cell[:32 * 7 + top] + b"\xff" + cell[32 * 7 + top + 1:]  # >= r in this mode's order alone
    other_order = bytearray(cell)
    other_order[32 * 9:32 * 9 + 32] = S.to_bytes(R, 1 - mode)            # r in the OTHER mode's order: below r in this one
    gen = oracle.g1_generator_mul(12345)
    bad = [
        (_x_off_the_curve(), k, cell, proof),                            # commitment: not a point
        (ORDER3, k, cell, proof),                                        # commitment: outside the subgroup
        (c, k, cell, _x_off_the_curve()),                                # proof: not a point
        (c, k, cell, bytes(48)),                                         # proof: not flagged compressed
        (c, k, cell[:64] + S.to_bytes(R, mode) + cell[96:], proof),      # an element equal to r
        (c, k, only_here, proof),
        (c, 128, cell, proof),
        (c, 1 << 63, cell, proof),
        (ORDER3, 128, cell, proof),                                      # a bad index and a bad point: the index decides
        (c, 200, cell[:2016] + b"\xff" * 32, _x_off_the_curve()),        # a bad index, a bad element and a bad proof
        (c, k, bytes(other_order), proof),                               # a value like any other: the call answers, and the answer is false
        (c, k, cell, INF),                                               # pi = infinity with C != infinity
    ]
    fine = [
        (INF, 77, bytes(2048), INF),                                     # C = pi = infinity with the zero cell
        (gen, 9, S.to_bytes(12345, mode) * 64, INF),                     # a constant polynomial: pi = infinity, C is not
    ]
    items, good_at = [], []
    for j, b in enumerate(bad + fine):
        good_at.append(len(items))
        items += [good[j % len(good)], b]
    good_at.append(len(items))
    items.append(good[-1])
    return items, good_at, len(bad)


@pytest.mark.parametrize("mode", MODES)
def test_every_answer_equals_the_batch_call_on_the_item_alone(K, gpu_setup, oracle, mode):
    items, good_at, n_bad = _mixed_batch(oracle, mode)
    assert 24 <= len(items) <= 32
    code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    with _mode(K, gpu_setup, mode):
        got = _each(K, gpu_setup, items)
        pts = _points(K, gpu_setup, items)
        for i, it in enumerate(items):
            assert got[i] == _rc(K, gpu_setup, [it]), i
    for i in good_at:
        assert got[i] == (K.C_KZG_OK, True), i                          # a good item's answer does not depend on its neighbours
    bad = [got[i] for i in range(1, 2 * n_bad, 2)]
    assert bad == [(code, False)] * 6 + [(K.C_KZG_BADARGS, False)] * 4 + [(K.C_KZG_OK, False)] * 2
    assert got[2 * n_bad + 1] == got[2 * n_bad + 3] == (K.C_KZG_OK, True)
    # the hook: a bad item did not reach the combine; C - I = O with pi = O is the point at infinity
    for j in range(10):
        assert pts[2 * j + 1] == b"\x02" + bytes(96), j
    assert pts[2 * n_bad + 1] == pts[2 * n_bad + 3] == b"\x01" + bytes(96)
    for i in good_at[:3] + [21, 23]:
        assert pts[i] == _want_point(oracle, items[i], mode, TAU), i


@pytest.mark.parametrize("mode", MODES)
def test_points_byte_for_byte_on_both_setups(K, gpu_setup, tau2_setup, oracle, mode):
    # k = 0, 1, 63, 64, 127: both sign branches of c_of_cell and the odd-exponent branch of cell_coeff_twist
    for ts, tau, seed in [(gpu_setup, TAU, 3000), (tau2_setup, M.TAU2, 3200)]:
        poly = Poly.seeded(oracle, seed, tau)
        items = [poly.item(k, mode) for k in (0, 1, 63, 64, 127)]
        items.append(items[1][:3] + (items[2][3],))                      # and a P that no pairing accepts
        with _mode(K, ts, mode):
            got = _points(K, ts, items)
            assert _each(K, ts, items) == [(K.C_KZG_OK, True)] * 5 + [(K.C_KZG_OK, False)]
        assert got == [_want_point(oracle, it, mode, tau) for it in items]
        assert all(p[0] == 0 for p in got)


def _low_degree_cases():
    """polynomials of degree < 64 (I_k = p for every cell): what the 64 lanes of k_celleach_commit hold before the tree, which pairs lane
    t with t + 1, then t + 2, ..."""
    x, t = 0x1234567890abcdef1234567890abcdef, TAU
    t2, t3 = t * t % R, t * t * t % R
    return {
        "lanes 0 and 1 equal": [x * t, x],
        "lanes 0 and 1 opposite": [-x * t, x],
        "lanes 2 and 3 equal": [0, 0, x * t, x],
        "lanes 2 and 3 opposite": [0, 0, -x * t, x],
        "two equal pairs": [x * t, x, x * t, x],
        "two opposite pairs": [-x * t, x, -x * t, x],
        "four equal lanes": [x * t3, x * t2, x * t, x],                   # the doubling branch at the first and at the second level
        "two pairs that cancel at the second level": [x * t3, x * t2, -x * t, -x],
        "equal lanes 62 and 63": [0] * 62 + [x * t, x],
        "constant": [12345],
        "zero": [],
    }


def test_the_reduction_trees_hard_cases(K, gpu_setup, oracle):
    mode = S.MODE_REFERENCE
    neighbour = Poly.seeded(oracle, 3000)
    items, wrong = [], []
    for name, low in _low_degree_cases().items():
        coeffs = [c % R for c in low] + [0] * (S.N_CELL - len(low))
        cm = oracle.g1_generator_mul(S.evaluate(coeffs, TAU))
        for k in (3, 100):
            cell = b"".join(S.to_bytes(S.evaluate(coeffs, xk), mode) for xk in S.coset_for_cell(k))
            items.append((cm, k, cell, INF))                             # the quotient by X^64 - c_k is zero: the honest proof is infinity
            wrong.append((cm, k, cell, neighbour.proof(k)))
    for it in items:
        assert V.interpolant_by_transform(V.cell_elements(it[2], mode), it[1])[4:62] == [0] * 58
    batch = items + wrong
    with _mode(K, gpu_setup, mode):
        got = _each(K, gpu_setup, batch)
        pts = _points(K, gpu_setup, batch)
    assert got == [(K.C_KZG_OK, True)] * len(items) + [(K.C_KZG_OK, False)] * len(wrong)
    assert pts == [_want_point(oracle, it, mode, TAU) for it in batch]
    assert pts[:len(items)] == [b"\x01" + bytes(96)] * len(items)


@pytest.mark.parametrize("mode", MODES)
def test_shapes_across_the_blocks_and_the_capacity_steps(K, gpu_setup, oracle, mode):
    # n = 64 | 65 and 128 | 130: a second block of k_celleach_combine and k_each_pairing, and the steps of the context's grow-only buffer
    # (64, 128, 256 items; no earlier call of this module is longer than 64); then a short call on the grown buffer
    two = [Poly.seeded(oracle, 3100 + j) for j in range(2)]
    pool = [p.item(k, mode) for p in two for k in range(128)]
    with _mode(K, gpu_setup, mode):
        for n in (1, 2, 63, 64, 65, 130, 3):
            honest = pool[:n] if n != 130 else pool[60:190]              # (the 130 cross from one polynomial into the other)
            batch, want = list(honest), [(K.C_KZG_OK, True)] * n
            for pos in {0, n - 1}:                                       # one corrupted item at the first and at the last position
                c, k, cell, _ = honest[pos]
                batch[pos] = (c, k, cell, honest[(pos + 1) % n][3] if n > 1 else pool[1][3])
                want[pos] = (K.C_KZG_OK, False)
            assert _each(K, gpu_setup, batch) == want, n


@pytest.mark.parametrize("mode", MODES)
def test_forms_streams_and_engines_agree(K, engine_setup, oracle, mode):
    import torch
    two = [Poly.seeded(oracle, 3100 + j) for j in range(2)]
    batch = [two[j % 2].item(j, mode) for j in range(65)]
    batch[0] = batch[0][:3] + (batch[1][3],)
    batch[17] = (batch[17][0], 128, batch[17][2], batch[17][3])
    batch[40] = (ORDER3,) + batch[40][1:]
    batch[64] = (batch[64][0], batch[64][1], batch[63][2], batch[64][3])
    code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    want = [(K.C_KZG_OK, True)] * 65
    want[0] = want[64] = (K.C_KZG_OK, False)
    want[17], want[40] = (K.C_KZG_BADARGS, False), (code, False)
    with _mode(K, engine_setup, mode):
        assert _each(K, engine_setup, batch) == want
        assert _device(K, engine_setup, batch) == want
        assert _device(K, engine_setup, batch, torch.cuda.Stream()) == want
        assert _each(K, engine_setup, batch) == want                    # a second call with the same inputs


def test_a_second_setup_in_the_same_process(K, gpu_setup, tau2_setup, oracle):
    mode = S.MODE_REFERENCE
    under_tau = [Poly.seeded(oracle, 3000).item(k, mode) for k in (5, 64)]
    under_tau2 = [Poly.seeded(oracle, 3200, M.TAU2).item(k, mode) for k in (5, 64)]
    both = under_tau + under_tau2
    for _ in range(2):                                                   # the line tables are the context's own, first use and later
        with _mode(K, gpu_setup, mode):
            assert [ok for _, ok in _each(K, gpu_setup, both)] == [True, True, False, False]
        with _mode(K, tau2_setup, mode):
            assert [ok for _, ok in _each(K, tau2_setup, both)] == [False, False, True, True]
