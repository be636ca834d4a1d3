"""GPU: per-group EIP-7594 cell proof verification (lwkzg_verify_cell_kzg_proof_groups, _device, lwkzg_cell_verify_groups_partials) in
reference and c-kzg mode, and once in eth mode. A group's answer is by definition lwkzg_verify_cell_kzg_proof_batch on its items alone,
so every (rc, ok) is held against that call on the range (which runs the bucket kernels of vmsm.hip, not the grouped call's), r and
the four sums of every group byte for byte against the restatement of tests/cell_verify_spec.py on both setups and against
lwkzg_cell_verify_partials on the range, and the verdicts against the check done in G1 with tau known. Honest items are made on the CPU
as tests/test_gpu_cell_verify.py makes them. The shapes cross the 64-term slices of all three sums, the 64-group chunk of the
interpolant kernels, the engine's launch set of MSM slots and the capacity steps of the context's buffer."""
import os
import re

import pytest

import cell_verify_spec as V
import cells_spec as S
import make_setups as M
from conftest import R, ROOT, SETUP_TAU2_PATH, TAU
from test_gpu_cell_verify import INF, MODES, Poly, _corruptions, _mode, _partials, _rc
from test_gpu_cell_verify_each import ORDER3, _low_degree_cases, _mixed_batch

pytestmark = pytest.mark.gpu

MODE_ETH = 2
ZERO = bytes(32 + 4 * 97)


def _csrc_constant(file, name):
    text = open(os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc", file)).read()
    return int(re.search(r"constexpr size_t %s = (\d+);" % name, text).group(1))


INTERP_CHUNK = _csrc_constant("cells_verify_groups.hip", "kInterpChunk")    # groups per pass of the interpolant kernels (64)
MSM_LAUNCH_SET = _csrc_constant("engine.h", "kMaxChunk")                    # the MSM workspace's slots per launch set (1024)


def _groups(K, ts, groups):
    return K.verify_cell_kzg_proof_groups(groups, ts)


def _gpartials(K, ts, groups):
    return K.cell_verify_groups_partials(groups, ts)


def _device(K, ts, groups, stream=None):
    """the device form; with a stream, the inputs are produced on it and nothing waits for them before the call"""
    import torch
    items = [it for grp in groups for it in grp]

    def dev(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(non_blocking=True)

    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        dc, dcell, dp = dev(b"".join(i[0] for i in items)), dev(b"".join(i[2] for i in items)), dev(b"".join(i[3] for i in items))
        di = torch.tensor([i[1] for i in items], dtype=torch.int64).cuda(non_blocking=True)
    if stream is None:
        torch.cuda.synchronize()
    got = K.verify_cell_kzg_proof_groups_device(dc.data_ptr(), di.data_ptr(), dcell.data_ptr(), dp.data_ptr(), len(items),
                                                [len(grp) for grp in groups], ts, None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    return got


def _bad_code(K, mode):
    return K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR


def _constant(oracle, c, k, mode):
    """the constant polynomial c: its commitment [c]G, any cell, and the honest proof, the point at infinity"""
    return (oracle.g1_generator_mul(c), k, S.to_bytes(c, mode) * 64, INF)


def _negated(point48):
    """the opposite of a compressed point that is not the point at infinity"""
    return bytes([point48[0] ^ 0x20]) + point48[1:]


def _pool(oracle, mode):
    two = [Poly.seeded(oracle, 3100 + j) for j in range(2)]
    return [p.item(k, mode) for p in two for k in range(128)]


@pytest.mark.parametrize("mode", MODES)
def test_partials_byte_for_byte_on_both_setups(K, gpu_setup, oracle, mode):
    # groups of 3, 2, 1, 6 and 64 items: a column of several blobs, several cells of one blob, one item, a repeated item with a
    # repeated commitment, and a full slice. The second setup lives for this test alone: nothing of it is left on the device behind it
    tau2_setup = K.TrustedSetup.from_file(SETUP_TAU2_PATH)
    try:
        _partials_on_both_setups(K, gpu_setup, tau2_setup, oracle, mode)
    finally:
        tau2_setup.free()


def _partials_on_both_setups(K, gpu_setup, tau2_setup, oracle, mode):
    for ts, tau, seed in [(gpu_setup, TAU, 3000), (tau2_setup, M.TAU2, 3200)]:
        polys = [Poly.seeded(oracle, seed + j, tau) for j in range(3)]
        few = [polys[j].item(k, mode) for j, k in [(0, 5), (1, 5), (0, 10)]]
        groups = [
            [p.item(5, mode) for p in polys],
            [polys[0].item(k, mode) for k in (10, 64)],
            [polys[1].item(127, mode)],
            few + [few[1], few[0], few[1]],
            [polys[0].item(k, mode) for k in range(64)],
        ]
        assert [len(grp) for grp in groups] == [3, 2, 1, 6, 64]
        with _mode(K, ts, mode):
            got = _gpartials(K, ts, groups)
            assert _groups(K, ts, groups) == [(K.C_KZG_OK, True)] * len(groups)
            alone = [_partials(K, ts, grp) for grp in groups]
        assert got == alone
        assert got == [V.partials_bytes(oracle, grp, mode, tau) for grp in groups]


@pytest.mark.parametrize("mode", MODES)
def test_every_answer_equals_the_batch_call_on_the_range_alone(K, gpu_setup, oracle, mode):
    items, good_at, n_bad = _mixed_batch(oracle, mode)
    good = [items[i] for i in good_at]
    n_fine = (len(items) - 1) // 2 - n_bad
    groups, kinds = [[]], ["empty"]
    for j in range(n_bad + n_fine):                       # one bad (or merely odd) item between two good ones, good groups between
        groups.append([good[j], items[2 * j + 1], good[j + 1]])
        kinds.append("bad" if j < n_bad else "fine")
        groups.append([good[j + 1], good[j]])
        kinds.append("good")
        if j % 5 == 2:
            groups.append([])
            kinds.append("empty")
    groups.append([(ORDER3,) + good[0][1:], (good[1][0], 128) + good[1][2:]])    # a bad index beats a bad point inside one group
    kinds.append("index")
    groups.append([])
    kinds.append("empty")
    code = _bad_code(K, mode)
    with _mode(K, gpu_setup, mode):
        got = _groups(K, gpu_setup, groups)
        part = _gpartials(K, gpu_setup, groups)
        for j, grp in enumerate(groups):
            assert got[j] == _rc(K, gpu_setup, grp), (j, kinds[j])
        for j, grp in enumerate(groups):
            if kinds[j] in ("good", "fine"):
                assert part[j] == _partials(K, gpu_setup, grp), j
    bad = [got[j] for j, kind in enumerate(kinds) if kind == "bad"]
    assert bad == [(code, False)] * 6 + [(K.C_KZG_BADARGS, False)] * 4 + [(K.C_KZG_OK, False)] * 2
    for j, kind in enumerate(kinds):
        if kind in ("good", "fine", "empty"):
            assert got[j] == (K.C_KZG_OK, True), (j, kind)      # a good group's answer does not depend on its neighbours
        if kind == "index":
            assert got[j] == (K.C_KZG_BADARGS, False)
        if kind in ("empty", "index") or (kind == "bad" and got[j][0] != K.C_KZG_OK):
            assert part[j] == ZERO, (j, kind)
        else:
            assert part[j] != ZERO, (j, kind)


@pytest.mark.parametrize("mode", MODES)
def test_verdicts_against_independent_truth(K, gpu_setup, oracle, mode):
    polys = [Poly.seeded(oracle, 3000 + j) for j in range(3)]
    honest = [[p.item(k, mode) for p in polys] for k in (5, 10, 64, 127)]
    three = [list(grp) for grp in honest]
    for n, name in enumerate(("neighbours_proof", "another_column", "cell_element")):
        where, pos = (n + 1) % 4, n                       # one corrupted item makes exactly its group false
        groups = [list(grp) for grp in honest]
        groups[where][pos] = three[(where + 1) % 4][pos] = _corruptions(honest[where][pos], polys, mode)[name]
        want = [V.verdict_known_tau(oracle, grp, mode, TAU) for grp in groups]
        assert want == [j != where for j in range(4)]
        with _mode(K, gpu_setup, mode):
            assert _groups(K, gpu_setup, groups) == [(K.C_KZG_OK, ok) for ok in want], name
    # and three of them in one call, each in a group it does not belong to either, around one honest group
    want = [V.verdict_known_tau(oracle, grp, mode, TAU) for grp in three]
    assert want == [False, True, False, False]
    with _mode(K, gpu_setup, mode):
        assert _groups(K, gpu_setup, three) == [(K.C_KZG_OK, ok) for ok in want]


def test_the_trees_hard_cases(K, gpu_setup, oracle):
    mode = S.MODE_REFERENCE
    p = Poly.seeded(oracle, 3000)
    groups, names = [], []
    for name, low in _low_degree_cases().items():         # honest proofs are the point at infinity: P and RLP of the group are, too
        coeffs = [c % R for c in low] + [0] * (S.N_CELL - len(low))
        cm = oracle.g1_generator_mul(S.evaluate(coeffs, TAU))
        groups.append([(cm, k, b"".join(S.to_bytes(S.evaluate(coeffs, xk), mode) for xk in S.coset_for_cell(k)), INF) for k in (3, 100)])
        names.append(name)
    a, b = p.item(7, mode), p.item(8, mode)
    groups += [
        [a, a],                                           # two equal proofs (and equal rows)
        [a, a[:3] + (_negated(a[3]),)],                   # two opposite proofs
        [_constant(oracle, 5, 1, mode), _constant(oracle, 6, 2, mode), _constant(oracle, 5, 3, mode)],   # infinity proofs alone
        [a[:3] + (INF,), b[:3] + (INF,)],                 # P is the point at infinity, the cells are not constant
        [a, b, _constant(oracle, 7, 9, mode)],            # an infinity lane beside two others
    ]
    names += ["equal proofs", "opposite proofs", "infinity proofs", "P at infinity", "one infinity lane"]
    with _mode(K, gpu_setup, mode):
        got = _groups(K, gpu_setup, groups)
        part = _gpartials(K, gpu_setup, groups)
        for j, grp in enumerate(groups):
            assert got[j] == _rc(K, gpu_setup, grp), names[j]
            assert part[j] == _partials(K, gpu_setup, grp), names[j]
    assert part == [V.partials_bytes(oracle, grp, mode, TAU) for grp in groups]
    want = [True] * len(_low_degree_cases()) + [True, False, True, False, True]
    assert got == [(K.C_KZG_OK, ok) for ok in want]
    for j, name in enumerate(names):
        if name not in ("equal proofs", "opposite proofs", "one infinity lane"):
            assert part[j][32] == 1 and part[j][32 + 3 * 97] == 1, name       # P and RLP


@pytest.mark.parametrize("mode", MODES)
def test_group_sizes_across_the_slices(K, gpu_setup, oracle, mode):
    # 63 | 64 | 65 | 128 | 129 items: one, two and three slices of the proofs' sums; the windows overlap (groups are independent)
    pool = _pool(oracle, mode)
    groups = [pool[0:63], pool[60:124], pool[100:165], pool[120:248], pool[127:256]]
    assert [len(grp) for grp in groups] == [63, 64, 65, 128, 129]
    bad = [list(grp) for grp in groups]
    for j, pos in [(2, 64), (4, 128), (1, 0)]:            # one corrupted item in the last slice of two groups, one in a first
        c, k, cell, _ = bad[j][pos]
        bad[j][pos] = (c, k, cell, bad[j][pos - 1][3])
    with _mode(K, gpu_setup, mode):
        assert _groups(K, gpu_setup, groups) == [(K.C_KZG_OK, True)] * 5
        assert _groups(K, gpu_setup, bad) == [(K.C_KZG_OK, ok) for ok in (True, False, False, True, False)]
        part = _gpartials(K, gpu_setup, bad)
        for j in (1, 2, 4):
            assert part[j] == _partials(K, gpu_setup, bad[j]), j
            assert _rc(K, gpu_setup, bad[j]) == (K.C_KZG_OK, False)


@pytest.mark.parametrize("mode", MODES)
def test_sixty_five_distinct_commitments_in_one_group(K, gpu_setup, oracle, mode):
    # the rows' sum RLC crosses a slice: 65 constant polynomials (a commitment each) and one item of a full one in front
    p = Poly.seeded(oracle, 3100)
    wide = [p.item(17, mode)] + [_constant(oracle, 1000 + j, (3 * j) % 128, mode) for j in range(65)]
    wrong = list(wide)
    wrong[65] = wrong[65][:2] + (S.to_bytes(999, mode) * 64,) + wrong[65][3:]      # row 65: the second slice
    groups = [wide, wrong, wide[:65]]
    with _mode(K, gpu_setup, mode):
        assert _groups(K, gpu_setup, groups) == [(K.C_KZG_OK, True), (K.C_KZG_OK, False), (K.C_KZG_OK, True)]
        part = _gpartials(K, gpu_setup, groups)
        for j, grp in enumerate(groups):
            assert part[j] == _partials(K, gpu_setup, grp), j


@pytest.mark.parametrize("mode", MODES)
def test_group_counts_across_the_chunks_and_the_capacity_steps(K, gpu_setup, oracle, mode):
    # g = 1, 2, 65 (one group past the interpolant kernels' chunk of 64) and 1025 (one past the engine's launch set of MSM slots) with
    # groups of one item, then a short call on the grown buffer. Four different items, one of them false, one with a bad index
    polys = [Poly.seeded(oracle, 3000 + j) for j in range(2)]
    a, b = polys[0].item(5, mode), polys[1].item(64, mode)
    kinds = [a, b, a[:3] + (b[3],), (a[0], 128) + a[2:]]
    with _mode(K, gpu_setup, mode):
        alone = [_rc(K, gpu_setup, [it]) for it in kinds]
        assert alone == [(K.C_KZG_OK, True), (K.C_KZG_OK, True), (K.C_KZG_OK, False), (K.C_KZG_BADARGS, False)]
        part_alone = [_partials(K, gpu_setup, [it]) for it in kinds[:3]] + [ZERO]
        for g in (1, 2, INTERP_CHUNK + 1, MSM_LAUNCH_SET + 1, 3):
            pick = [(5 * j + j // 64 + j // 1024) % 4 for j in range(g)]
            pick[-1] = 2                                     # the group behind each boundary answers false
            groups = [[kinds[q]] for q in pick]
            assert _groups(K, gpu_setup, groups) == [alone[q] for q in pick], g
            if g <= INTERP_CHUNK + 1:
                assert _gpartials(K, gpu_setup, groups) == [part_alone[q] for q in pick], g


@pytest.mark.parametrize("mode", MODES)
def test_forms_streams_and_engines_agree(K, gpu_setup, bucket_setup, oracle, mode):
    # both engines the engine_setup fixture hands out, one after the other
    for engine_setup in (gpu_setup, bucket_setup):
        _forms_and_streams_agree(K, engine_setup, oracle, mode)


def _forms_and_streams_agree(K, engine_setup, oracle, mode):
    import torch
    pool = _pool(oracle, mode)
    groups = [pool[0:3], [], pool[3:70], pool[128:130], pool[130:131], pool[200:256], []]
    groups[0][1] = groups[0][1][:3] + (groups[0][0][3],)
    groups[3][1] = (groups[3][1][0], 128) + groups[3][1][2:]
    groups[5][40] = (ORDER3,) + groups[5][40][1:]
    want = [(K.C_KZG_OK, False), (K.C_KZG_OK, True), (K.C_KZG_OK, True), (K.C_KZG_BADARGS, False), (K.C_KZG_OK, True),
            (_bad_code(K, mode), False), (K.C_KZG_OK, True)]
    with _mode(K, engine_setup, mode):
        assert _groups(K, engine_setup, groups) == want
        assert _device(K, engine_setup, groups) == want
        assert _device(K, engine_setup, groups, torch.cuda.Stream()) == want
        assert _groups(K, engine_setup, groups) == want                  # a second call with the same inputs
        assert _rc(K, engine_setup, groups[2]) == want[2] and _rc(K, engine_setup, groups[0]) == want[0]


def test_eth_mode_against_the_librarys_own_partials(K, gpu_setup, oracle):
    # eth mode's cells are big-endian elements, as reference mode's: the same items, answered by the third mode's rules
    pool = _pool(oracle, S.MODE_REFERENCE)
    groups = [pool[0:5], [], pool[120:190], pool[5:7], pool[7:9]]
    groups[3][0] = groups[3][0][:3] + (groups[3][1][3],)
    groups[4][1] = groups[4][1][:2] + (b"\xff" + groups[4][1][2][1:],) + groups[4][1][3:]     # an element not below r
    with _mode(K, gpu_setup, MODE_ETH):
        got = _groups(K, gpu_setup, groups)
        part = _gpartials(K, gpu_setup, groups)
        for j, grp in enumerate(groups):
            assert got[j] == _rc(K, gpu_setup, grp), j
        for j in (0, 2, 3):
            assert part[j] == _partials(K, gpu_setup, groups[j]), j
            assert part[j][:32] == K.cell_batch_challenge_host(*[[it[q] for it in groups[j]] for q in range(4)], MODE_ETH)
    assert got == [(K.C_KZG_OK, True), (K.C_KZG_OK, True), (K.C_KZG_OK, True), (K.C_KZG_OK, False), (K.C_KZG_BADARGS, False)]
    assert part[1] == part[4] == ZERO
