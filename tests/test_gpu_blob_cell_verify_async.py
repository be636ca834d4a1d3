"""GPU: cell proofs of whole blobs on the cell verifier that does not block -- lwkzg_cell_verifier_new_blobs / _enqueue_blobs /
_enqueue_blobs_groups and the blob-level grouping and expansion kernels behind them. The reference is always the
synchronous lwkzg_verify_blob_cell_kzg_proofs_batch_device / _groups_device and the partials hooks in the same process, compared byte
for byte; the grouping hook is held against plan_blobs / blob_item_lists (cell_blobs_plan.h) restated here. The blobs are the six
library-made ones per mode of test_gpu_blob_cell_verify.Made, and one polynomial the library did not make."""
import ctypes as C
import random

import pytest

import cells_spec as S
from conftest import R, SETUP_PATH
from test_gpu_blob_cell_verify import CELLS, MODES, MODE_ETH, ORDER3, Made, _bad_code, _blob_of, _el, _groups_device, _items, _mode, _rc_device
from test_gpu_cell_verify import Poly
from test_gpu_cell_verify_async import NONE_BAD, _Dev, _long_work

pytestmark = pytest.mark.gpu

MAX_BLOBS, MAX_GROUPS = 65, 8
ZERO = bytes(32 + 4 * 97)
SEVEN = ([1, 0, 0, 2, 1, 0, 2], [0, 3, 0, 4, 0])
SHAPES = {"one": ([0], [1]), "same_blob_twice": ([0, 0], [2]), "A_B_A": ([0, 1, 0], [2, 1]), "seven": SEVEN}
GOOD = (0, True)


@pytest.fixture(scope="module")
def verifier(K, gpu_setup):
    v = K.CellVerifier.for_blobs(gpu_setup, MAX_BLOBS, MAX_GROUPS)
    yield v
    v.free()


class _D:
    """the three arrays of a blob call on the device"""

    def __init__(self, blobs, comms, proofs):
        import torch

        def dev(data):
            return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()

        self.n = len(blobs)
        self.db, self.dc, self.dp = dev(b"".join(blobs)), dev(b"".join(comms)), dev(b"".join(proofs))
        torch.cuda.synchronize()

    def ptrs(self):
        return self.db.data_ptr(), self.dc.data_ptr(), self.dp.data_ptr()


def _cut(xs, sizes):
    out, at = [], 0
    for m in sizes:
        out.append(xs[at:at + m])
        at += m
    return out


def _fields(res):
    return res.state, res.rc, res.ok, res.first_bad, res.m


def _batch(v, call, stream=None):
    d = _D(*call)
    res = v.enqueue_blobs(*d.ptrs(), d.n, stream)
    v.wait()
    assert res.state == 1 and v.pending() == 0
    return res


def _groups(v, call, sizes, stream=None):
    d = _D(*call)
    ans = v.enqueue_blobs_groups(*d.ptrs(), d.n, sizes, stream)
    v.wait()
    assert ans.result.state == 1 and v.pending() == 0
    return ans


def _check_equal_to_the_synchronous_calls(K, ts, v, made, order, sizes):
    """an honest call: the batch's and the groups' partials byte for byte, the answers, and the results' fields"""
    call = made.call(order)
    blobs, comms, proofs = call
    res = _batch(v, call)
    want = K.blob_cell_verify_partials(blobs, comms, proofs, ts)
    cm, idx, cells, pf = made.expanded(blobs, comms, proofs)
    print("batch", order, _fields(res))
    assert bytes(res.partials) == want == K.cell_verify_partials(cm, idx, cells, pf, ts)
    assert _fields(res) == (1, K.C_KZG_OK, 1, NONE_BAD, len(set(order)))
    assert _rc_device(K, ts, blobs, comms, proofs) == (K.C_KZG_OK, True)
    ans = _groups(v, call, sizes)
    want_g = K.blob_cell_verify_groups_partials(blobs, comms, proofs, sizes, ts)
    print("groups", sizes, ans.answers(), _fields(ans.result))
    assert ans.partials() == want_g
    assert ans.answers() == _groups_device(K, ts, blobs, comms, proofs, sizes) == [(K.C_KZG_OK, True)] * len(sizes)
    assert _fields(ans.result) == (1, K.C_KZG_OK, 1, NONE_BAD, sum(len(set(grp)) for grp in _cut(order, sizes)))
    assert bytes(ans.result.partials) == ZERO
    assert [p != ZERO for p in want_g] == [m > 0 for m in sizes]


# ---- 1, 2: equality with the synchronous forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_results_equal_the_synchronous_forms(K, gpu_setup, verifier, mode, shape):
    made = Made.of(K, gpu_setup, mode)
    with _mode(K, gpu_setup, mode):
        _check_equal_to_the_synchronous_calls(K, gpu_setup, verifier, made, *SHAPES[shape])


@pytest.mark.parametrize("mode", [S.MODE_REFERENCE, MODE_ETH])
def test_sixty_five_blobs_of_three_commitments(K, gpu_setup, verifier, mode):
    """more than 64 blobs in a group, the verifier full, and the slice table beyond one slice per sum"""
    made = Made.of(K, gpu_setup, mode)
    with _mode(K, gpu_setup, mode):
        _check_equal_to_the_synchronous_calls(K, gpu_setup, verifier, made, [j % 3 for j in range(65)], [1, 0, 64])


# ---- 3: honest inputs that the library did not make -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_an_honest_polynomial_over_the_known_tau_answers_true(K, gpu_setup, verifier, oracle, mode):
    poly = Poly.seeded(oracle, 3100)
    blob, proofs = _blob_of(poly.p, mode), b"".join(poly.proof(k) for k in range(CELLS))
    swapped = proofs[48:96] + proofs[:48] + proofs[96:]
    with _mode(K, gpu_setup, mode):
        res = _batch(verifier, ([blob], [poly.cm], [proofs]))
        assert (res.rc, res.ok, res.first_bad, res.m) == (K.C_KZG_OK, 1, NONE_BAD, 1)
        assert _groups(verifier, ([blob], [poly.cm], [proofs]), [1]).answers() == [(K.C_KZG_OK, True)]
        res = _batch(verifier, ([blob], [poly.cm], [swapped]))
        assert (res.rc, res.ok, res.first_bad) == (K.C_KZG_OK, 0, NONE_BAD)
        assert _groups(verifier, ([blob], [poly.cm], [swapped]), [1]).answers() == [(K.C_KZG_OK, False)]


# ---- 4: single corruptions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_single_corruptions_change_exactly_one_group(K, gpu_setup, verifier, mode):
    made = Made.of(K, gpu_setup, mode)
    blobs, comms, proofs = made.call([0, 1, 2])
    sizes = [1, 2]
    code = _bad_code(K, mode)
    low = 0 if mode == S.MODE_CKZG else 31
    at = 32 * 1234 + low
    pf1 = proofs[1]
    equal_r = blobs[2][:32 * 4095] + _el(R, mode) + blobs[2][32 * 4096:]
    cases = [
        ("a proof of another blob", (blobs, comms, [proofs[0], pf1[:48 * 5] + made.proofs[3][48 * 5:48 * 6] + pf1[48 * 6:], proofs[2]]),
         1, (K.C_KZG_OK, False), NONE_BAD),
        ("one blob byte", ([blobs[0][:at] + bytes([blobs[0][at] ^ 1]) + blobs[0][at + 1:]] + blobs[1:], comms, proofs), 0, (K.C_KZG_OK, False), NONE_BAD),
        ("an order-3 proof", (blobs, comms, [proofs[0], pf1[:48 * 5] + ORDER3 + pf1[48 * 6:], proofs[2]]), 1, (code, False), 128 + 5),
        ("an order-3 commitment", (blobs, [comms[0], ORDER3, ORDER3], proofs), 1, (code, False), 128),
        ("an element equal to r", (blobs[:2] + [equal_r], comms, proofs), 1,
         (K.C_KZG_OK, False) if mode == S.MODE_REFERENCE else (code, False), NONE_BAD if mode == S.MODE_REFERENCE else 256)]
    with _mode(K, gpu_setup, mode):
        honest = K.blob_cell_verify_groups_partials(blobs, comms, proofs, sizes, gpu_setup)
        for name, call, group, answer, first_bad in cases:
            want = [GOOD, GOOD]
            want[group] = answer
            ans = _groups(verifier, call, sizes)
            res = _batch(verifier, call)
            print(name, ans.answers(), _fields(ans.result), _fields(res))
            assert ans.answers() == want == _groups_device(K, gpu_setup, *call, sizes), name
            assert (ans.result.rc, ans.result.ok, ans.result.first_bad) == (K.C_KZG_OK, 0, group), name
            got = ans.partials()
            assert got[1 - group] == honest[1 - group] and got[group] != honest[group], name
            if answer[0] != K.C_KZG_OK:
                assert got[group] == ZERO, name      # nothing behind r ran on the group
            assert (res.rc, bool(res.ok)) == answer == _rc_device(K, gpu_setup, *call), name
            assert res.first_bad == first_bad, name
            if answer[0] != K.C_KZG_OK:
                assert bytes(res.partials) == ZERO, name
        # nothing is stale
        res = _batch(verifier, (blobs, comms, proofs))
        assert _fields(res) == (1, K.C_KZG_OK, 1, NONE_BAD, 3)
        ans = _groups(verifier, (blobs, comms, proofs), sizes)
        assert ans.answers() == [GOOD, GOOD] and ans.partials() == honest


# ---- 5: the grouping hook against the plan ---------------------------------------------------------------------------------------------------
def _plan(comms, sizes):
    """plan_blobs and blob_item_lists (cell_blobs_plan.h) restated for the 128 n expanded items: rows, row_base, the concatenated distinct
    commitments, first_item, item_group, idx, the row and (group, column) lists as sets, and the slice table"""
    n = CELLS * len(comms)
    p = {"rows": [], "row_base": [0], "distinct": [], "first_item": [], "item_group": [], "row_sets": [], "col_sets": [], "slices": [],
         "slice_off": [0], "bad_words": [0] * len(sizes), "idx": list(range(CELLS)) * len(comms)}
    lo = 0
    for j, m in enumerate(sizes):
        seen = {}
        for b in range(lo, lo + m):
            if comms[b] not in seen:
                seen[comms[b]] = len(seen)
                p["distinct"].append(comms[b])
                p["first_item"].append(CELLS * b)
                p["row_sets"].append(set())
            p["rows"] += [seen[comms[b]]] * CELLS
            p["item_group"] += [j] * CELLS
            p["row_sets"][p["row_base"][-1] + seen[comms[b]]].update(range(CELLS * b, CELLS * b + CELLS))
        p["col_sets"] += [{CELLS * b + k for b in range(lo, lo + m)} for k in range(CELLS)]
        for s, (first, count) in enumerate([(CELLS * lo, CELLS * m), (CELLS * lo, CELLS * m), (p["row_base"][-1], len(seen))]):
            p["slices"] += [(j, s, first + at, min(64, count - at)) for at in range(0, count, 64)]
            p["slice_off"].append(len(p["slices"]))
        p["row_base"].append(p["row_base"][-1] + len(seen))
        lo += m
    p["m"] = p["row_base"][-1]
    p["distinct"] = b"".join(p["distinct"]) + (bytes([0xc0]) + bytes(47)) * (n - p["m"])
    return p


def _sets(perm, off):
    return [set(perm[off[q]:off[q + 1]]) for q in range(len(off) - 1)]


def _hook_cases():
    rnd = random.Random(4242)
    strings = [bytes(rnd.randrange(256) for _ in range(48)) for _ in range(300)]
    three = [bytes([0xa0 + t]) * 48 for t in range(3)]
    full = strings + [strings[rnd.randrange(300)] for _ in range(212)]
    return {"one blob": ([three[0]], [1]),
            "seven": ([three[t] for t in SEVEN[0]], SEVEN[1]),
            "70 distinct in one group": (strings[:70], [70]),
            "512 blobs of 300 strings in 5 groups": (full, [200, 0, 100, 12, 200])}


@pytest.mark.parametrize("hash_mask", [0, 0xffffffff], ids=["one_chain", "spread"])
def test_blob_grouping_hook_against_the_plan_restated(K, gpu_setup, hash_mask):
    """every key on one probe chain (hash_mask 0) and spread; the hook needs no valid points. The order inside a row's list and inside a
    (group, column) list is undefined: compared as sets"""
    import torch
    for name, (comms, sizes) in _hook_cases().items():
        n = CELLS * len(comms)
        dc = torch.frombuffer(bytearray(b"".join(comms)), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        got = K.blob_group_device(dc.data_ptr(), len(comms), sizes, 0x1234, hash_mask)
        want = _plan(comms, sizes)
        for key in ("m", "rows", "row_base", "bad_words", "distinct", "first_item", "item_group", "idx", "slice_off", "slices"):
            assert got[key] == want[key], (name, key)
        assert got["row_off"][0] == 0 and got["row_off"][-1] == n and got["col_off"][0] == 0 and got["col_off"][-1] == n, name
        assert _sets(got["perm_row"], got["row_off"]) == want["row_sets"], name
        assert _sets(got["perm_col"], got["col_off"]) == want["col_sets"], name
        if name == "seven":     # and the item-level segmented grouping on the expanded commitments and indices
            items = torch.frombuffer(bytearray(b"".join(c * CELLS for c in comms)), dtype=torch.uint8).cuda()
            idx = torch.tensor(want["idx"], dtype=torch.int64).cuda()
            torch.cuda.synchronize()
            seg = K.cell_group_segmented_device(items.data_ptr(), idx.data_ptr(), n, [CELLS * m for m in sizes], 0x1234, hash_mask)
            for key in ("m", "rows", "row_base", "bad_words", "distinct", "first_item", "row_off", "col_off", "slice_off", "slices"):
                assert got[key] == seg[key], (name, key)
            assert _sets(got["perm_row"], got["row_off"]) == _sets(seg["perm_row"], seg["row_off"])
            assert _sets(got["perm_col"], got["col_off"]) == _sets(seg["perm_col"], seg["col_off"])


# ---- 6, 7: the shell ---------------------------------------------------------------------------------------------------------------------------
def test_enqueue_returns_without_waiting_and_the_answers_are_in_stream_order(K, gpu_setup, verifier):
    """long work queued ahead on the caller's stream: enqueue_blobs_groups returns with the result pending and the stream busy. A proof
    overwritten on the stream behind the first call does not reach it, and reaches the second"""
    import torch
    made = Made.of(K, gpu_setup, S.MODE_REFERENCE)
    d = _D(*made.call([0, 1, 2]))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _mode(K, gpu_setup, S.MODE_REFERENCE):
        _long_work(torch, st)
        first = verifier.enqueue_blobs_groups(*d.ptrs(), 3, [1, 2], st.cuda_stream)
        state, pending, drained = first.result.state, verifier.pending(), st.query()
        with torch.cuda.stream(st):
            at = 48 * (CELLS + 27)
            d.dp[at:at + 48] = d.dp[48 * 3:48 * 4].clone()   # ordered behind the first call: enqueue joins its end into the stream
        second = verifier.enqueue_blobs_groups(*d.ptrs(), 3, [1, 2], st.cuda_stream)
        assert (state, pending, drained) == (0, 1, False)
        st.synchronize()                                     # the stream was ordered behind both calls: no wait on the verifier
        assert (first.result.state, second.result.state) == (1, 1)
        verifier.wait()
    assert first.answers() == [GOOD, GOOD] and second.answers() == [GOOD, (0, False)]
    assert (second.result.ok, second.result.first_bad) == (0, 1)


def test_depth_plus_two_calls_back_to_back_all_four_kinds_in_turn(K, gpu_setup, verifier):
    mode = S.MODE_REFERENCE
    made = Made.of(K, gpu_setup, mode)
    blobs, comms, proofs = made.call([0, 1, 2])
    bad_proofs = proofs[:2] + [proofs[2][:48 * 9] + proofs[2][48 * 10:48 * 11] + proofs[2][48 * 10:]]     # item 265, of group 1
    cm, idx, cells, pf = made.expanded(blobs, comms, proofs)
    items = _items(cm, idx, cells, pf, 0, 3 * CELLS)
    bad_items = _items(cm, idx, cells, b"".join(bad_proofs), 0, 3 * CELLS)
    good_b, bad_b, good_i, bad_i = _D(blobs, comms, proofs), _D(blobs, comms, bad_proofs), _Dev(items), _Dev(bad_items)
    calls, seen = [], []
    with _mode(K, gpu_setup, mode):
        for q in range(K.VERIFIER_DEPTH + 2):
            bad = q % 3 == 2
            kind = q % 4
            if kind == 0:
                d = bad_b if bad else good_b
                calls.append(verifier.enqueue_blobs(*d.ptrs(), 3))
            elif kind == 1:
                d = bad_i if bad else good_i
                calls.append(verifier.enqueue(*d.ptrs(), d.n))
            elif kind == 2:
                d = bad_b if bad else good_b
                calls.append(verifier.enqueue_blobs_groups(*d.ptrs(), 3, [1, 2]))
            else:
                d = bad_i if bad else good_i
                calls.append(verifier.enqueue_groups(*d.ptrs(), d.n, [CELLS, 2 * CELLS]))
            seen.append(verifier.pending())
        verifier.wait()
    assert max(seen) <= K.VERIFIER_DEPTH and min(seen) >= 0, seen
    for q, c in enumerate(calls):
        ok = q % 3 != 2
        if q % 4 in (2, 3):
            assert c.answers() == [GOOD, (0, ok)] and (c.result.state, c.result.rc, c.result.ok) == (1, 0, int(ok)), q
        else:
            assert (c.state, c.rc, c.ok, c.m) == (1, 0, int(ok), 3), q


# ---- 8: completions on the spot --------------------------------------------------------------------------------------------------------------
def test_completions_on_the_spot(K, gpu_setup, verifier):
    made = Made.of(K, gpu_setup, S.MODE_REFERENCE)
    d = _D(*made.call([0, 1, 2]))
    l = K.lib()
    filled = b"\x11" * (4 * len(ZERO))

    def groups(v, ptrs, n, offsets, g, ok=True, rc=True, written=False):
        res = K.CellVerifyResult()
        res.state, res.rc, res.ok = 9, 9, 9
        okb, rcb, part = (C.c_uint8 * 4)(7, 7, 7, 7), (C.c_int32 * 4)(-5, -5, -5, -5), C.create_string_buffer(filled, len(filled))
        off = (C.c_uint64 * len(offsets))(*offsets) if offsets is not None else None
        got = l.lwkzg_cell_verifier_enqueue_blobs_groups(v.h, C.byref(res), okb if ok else None, rcb if rc else None, part, *ptrs, n, off, g, None)
        if not written:
            assert list(okb) == [7] * 4 and list(rcb) == [-5] * 4 and part.raw == filled      # nothing but *result is written
        assert v.pending() == 0
        return got, _fields(res), (list(okb), list(rcb), part.raw)

    def batch(v, ptrs, n):
        res = K.CellVerifyResult()
        res.state, res.rc, res.ok = 9, 9, 9
        got = l.lwkzg_cell_verifier_enqueue_blobs(v.h, C.byref(res), *ptrs, n, None)
        assert v.pending() == 0
        return got, _fields(res), bytes(res.partials)

    refused = (K.C_KZG_BADARGS, (1, K.C_KZG_BADARGS, 0, NONE_BAD, 0))
    empty = (K.C_KZG_OK, (1, K.C_KZG_OK, 1, NONE_BAD, 0))
    for mode in MODES:      # n == 0, in every mode
        with _mode(K, gpu_setup, mode):
            assert batch(verifier, (None,) * 3, 0) == empty + (ZERO,)
    with _mode(K, gpu_setup, S.MODE_REFERENCE):
        # g == 0 with n == 0; empty groups alone
        assert groups(verifier, (None,) * 3, 0, None, 0)[:2] == empty
        got = groups(verifier, (None,) * 3, 0, [0, 0, 0], 2, written=True)
        assert got[:2] == empty
        assert got[2] == ([1, 1, 7, 7], [0, 0, -5, -5], bytes(2 * len(ZERO)) + filled[2 * len(ZERO):])
        # n above max_blobs, g above max_groups, bad offsets, g == 0 with n > 0
        assert batch(verifier, d.ptrs(), MAX_BLOBS + 1)[:2] == refused
        assert groups(verifier, d.ptrs(), MAX_BLOBS + 1, [0, MAX_BLOBS + 1], 1)[:2] == refused
        assert groups(verifier, d.ptrs(), 3, [0] * MAX_GROUPS + [1, 3], MAX_GROUPS + 1)[:2] == refused
        for off in ([1, 3], [0, 2, 1, 3], [0, 384]):
            assert groups(verifier, d.ptrs(), 3, off, len(off) - 1)[:2] == refused, off
        assert groups(verifier, d.ptrs(), 3, [0], 0)[:2] == refused
        # each NULL argument
        for missing in range(3):
            ptrs = list(d.ptrs())
            ptrs[missing] = None
            assert batch(verifier, ptrs, 3)[:2] == refused, missing
            assert groups(verifier, ptrs, 3, [0, 1, 3], 2)[:2] == refused, missing
        assert groups(verifier, d.ptrs(), 3, None, 2)[:2] == refused
        assert groups(verifier, d.ptrs(), 3, [0, 1, 3], 2, ok=False)[:2] == refused
        assert groups(verifier, d.ptrs(), 3, [0, 1, 3], 2, rc=False)[:2] == refused
        res = K.CellVerifyResult()
        assert l.lwkzg_cell_verifier_enqueue_blobs(None, C.byref(res), *d.ptrs(), 3, None) == K.C_KZG_BADARGS and res.state == 1
        assert l.lwkzg_cell_verifier_enqueue_blobs(verifier.h, None, *d.ptrs(), 3, None) == K.C_KZG_BADARGS
        # a verifier without blob scratch says why; one without groups refuses a grouped blob call
        items, no_groups = K.CellVerifier(gpu_setup, 256, 2), K.CellVerifier.for_blobs(gpu_setup, 3)
        try:
            assert batch(items, d.ptrs(), 1)[:2] == refused
            assert b"lwkzg_cell_verifier_new_blobs" in l.lwkzg_last_error()
            assert groups(items, d.ptrs(), 1, [0, 1], 1)[:2] == refused
            assert groups(no_groups, d.ptrs(), 3, [0, 1, 3], 2)[:2] == refused
            res = no_groups.enqueue_blobs(*d.ptrs(), 3)       # and it works as a batch verifier of blobs, full
            no_groups.wait()
            assert _fields(res) == (1, K.C_KZG_OK, 1, NONE_BAD, 3)
        finally:
            items.free()
            no_groups.free()
        for max_blobs in (0, 513):
            with pytest.raises(K.KzgError) as e:
                K.CellVerifier.for_blobs(gpu_setup, max_blobs, 1)
            assert e.value.rc == K.C_KZG_BADARGS


# ---- 9: no allocation in steady state -------------------------------------------------------------------------------------------------------
def test_a_second_call_allocates_nothing(K, gpu_setup, verifier):
    import torch
    made = Made.of(K, gpu_setup, MODE_ETH)
    d = _D(*made.call(range(6)))
    with _mode(K, gpu_setup, MODE_ETH):
        for call in (lambda: verifier.enqueue_blobs(*d.ptrs(), 6), lambda: verifier.enqueue_blobs_groups(*d.ptrs(), 6, [1, 0, 2, 3]).result):
            first = call()
            verifier.wait()
            torch.cuda.synchronize()
            free = torch.cuda.mem_get_info()[0]      # hipMemGetInfo
            second = call()
            verifier.wait()
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free
            assert _fields(first) == _fields(second) and first.ok == 1


# ---- 10: a setup freed under a verifier --------------------------------------------------------------------------------------------------------
def test_setup_freed_under_a_verifier(K, gpu_setup):
    """free_trusted_setup waits for the blob call in flight; the verifier then refuses, and is still freed cleanly"""
    made = Made.of(K, gpu_setup, S.MODE_REFERENCE)
    d = _D(*made.call([0, 1, 0]))
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    ts.set_mode(K.MODE_REFERENCE)
    v = K.CellVerifier.for_blobs(ts, 4, 2)
    ans = v.enqueue_blobs_groups(*d.ptrs(), 3, [2, 1])
    ts.free()
    assert _fields(ans.result) == (1, 0, 1, NONE_BAD, 3) and ans.answers() == [GOOD, GOOD]
    for call in (lambda: v.enqueue_blobs(*d.ptrs(), 3), lambda: v.enqueue_blobs_groups(*d.ptrs(), 3, [2, 1])):
        with pytest.raises(K.KzgError) as e:
            call()
        assert e.value.rc == K.C_KZG_BADARGS and e.value.result.state == 1
    v.free()
    assert v.pending() == -1


# ---- 11: both engines ------------------------------------------------------------------------------------------------------------------------
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
    v = K.CellVerifier.for_blobs(ts, 3, 2)
    try:
        with _mode(K, ts, mode):
            _check_equal_to_the_synchronous_calls(K, ts, v, made, *SHAPES["A_B_A"])
    finally:
        v.free()
