"""GPU: per-group cell proof verdicts that do not block the caller -- lwkzg_cell_verifier_new_groups / _enqueue_groups and the segmented
grouping kernels behind them. The reference is always the synchronous lwkzg_verify_cell_kzg_proof_groups_device
plus lwkzg_cell_verify_groups_partials in the same process, compared byte for byte; the segmented-grouping hook is held against a plain
restatement of plan_groups (cell_groups_plan.h). The cells are the library's own: the 128 cells of nine blobs per mode."""
import pytest

import blobs as B
import cells_spec as S
from conftest import R, SETUP_PATH
from test_gpu_cell_verify import MODES, _mode, _rc, _x_off_the_curve
from test_gpu_cell_verify_async import NONE_BAD, _Dev, _long_work

pytestmark = pytest.mark.gpu

CAP, GCAP = 1152, 72
ZERO = bytes(32 + 4 * 97)
ORDER3 = bytes([0x80]) + bytes(47)            # (0, 2): on the curve, of order 3
BOUNDARY_SIZES = [0, 1, 2, 63, 0, 64, 65, 130, 0]   # 64: the slice length; 130: three slices; empty groups in front, inside, behind


@pytest.fixture(scope="module")
def library_cells(K, gpu_setup):
    """the 128 cells of nine blobs with their proofs, made by the library: 1152 items per mode, blob after blob"""
    out = {}
    for mode in MODES:
        blobs = b"".join(B.synthetic_blob(960 + i, big_endian=mode == S.MODE_REFERENCE) for i in range(9))
        with _mode(K, gpu_setup, mode):
            comms = K.blob_to_kzg_commitment_batch(blobs, gpu_setup)
            made = K.compute_cells_and_kzg_proofs_batch(blobs, gpu_setup)
        out[mode] = [(comms[b], k, made[b][0][k], made[b][1][k]) for b in range(9) for k in range(128)]
    return out


@pytest.fixture(scope="module")
def verifier(K, gpu_setup):
    v = K.CellVerifier(gpu_setup, CAP, GCAP)
    yield v
    v.free()


def _cut(items, sizes):
    assert sum(sizes) <= len(items)
    out, at = [], 0
    for m in sizes:
        out.append(items[at:at + m])
        at += m
    return out


def _rows(groups):
    """per group the number of distinct commitments, 0 for a group with an index >= 128"""
    return [0 if any(i[1] >= 128 for i in grp) else len({i[0] for i in grp}) for grp in groups]


def _same_as_the_synchronous_call(K, ts, v, groups, name=None, stream=None):
    """every group's (rc, ok) and partials byte for byte, and the result's fields; returns the answers"""
    d = _Dev([it for grp in groups for it in grp])
    sizes = [len(grp) for grp in groups]
    ans = v.enqueue_groups(*d.ptrs(), d.n, sizes, stream)
    v.wait()
    res = ans.result
    assert res.state == 1 and v.pending() == 0, name
    want = K.verify_cell_kzg_proof_groups_device(*d.ptrs(), d.n, sizes, ts)
    want_partials = K.cell_verify_groups_partials(groups, ts)
    got, got_partials = ans.answers(), ans.partials()
    print(name, "answers", got, "m", res.m, "first_bad", res.first_bad)
    assert got == want, name
    assert got_partials == want_partials, (name, [j for j in range(len(groups)) if got_partials[j] != want_partials[j]])
    bad = [j for j, a in enumerate(want) if a != (K.C_KZG_OK, True)]
    assert (res.rc, res.ok, res.first_bad) == (K.C_KZG_OK, 0 if bad else 1, bad[0] if bad else NONE_BAD), name
    assert res.m == sum(_rows(groups)) and bytes(res.partials) == ZERO, name
    return got, got_partials


# ---- honest calls: group sizes at the boundaries ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_group_sizes_at_the_boundaries_in_one_call(K, gpu_setup, verifier, library_cells, mode):
    groups = _cut(library_cells[mode], BOUNDARY_SIZES)
    with _mode(K, gpu_setup, mode):
        got, partials = _same_as_the_synchronous_call(K, gpu_setup, verifier, groups, "boundaries")
    assert got == [(K.C_KZG_OK, True)] * len(groups)
    assert [p != ZERO for p in partials] == [m > 0 for m in BOUNDARY_SIZES]


@pytest.mark.parametrize("mode", MODES)
def test_sixty_five_groups_of_one_item(K, gpu_setup, verifier, library_cells, mode):
    items = library_cells[mode][100:165]       # across two blobs
    with _mode(K, gpu_setup, mode):
        got, _ = _same_as_the_synchronous_call(K, gpu_setup, verifier, [[it] for it in items], "65 x 1")
    assert got == [(K.C_KZG_OK, True)] * 65


@pytest.mark.parametrize("mode", MODES)
def test_flagged_groups_in_the_second_interpolant_chunk(K, gpu_setup, verifier, library_cells, mode):
    """66 groups of one item: groups 64 and 65 are the second chunk of the interpolant kernels (first = 64), whose workgroups read their
    group's flag at first + blockIdx.y. Group 64 has the index 128, group 65 a proof with one byte changed; every group answers as the
    batch call on its item alone, through enqueue_groups and through the synchronous grouped call"""
    items = list(library_cells[mode][200:266])
    items[64] = (items[64][0], 128) + items[64][2:]
    proof = items[65][3]
    items[65] = items[65][:3] + (proof[:47] + bytes([proof[47] ^ 1]),)
    groups = [[it] for it in items]
    with _mode(K, gpu_setup, mode):
        got, _ = _same_as_the_synchronous_call(K, gpu_setup, verifier, groups, "66 x 1, flags in the second chunk")
        alone = [_rc(K, gpu_setup, grp) for grp in groups]
    print("groups 64, 65:", got[64:], "alone:", alone[64:])
    assert got == alone
    assert got[:64] == [(K.C_KZG_OK, True)] * 64
    assert got[64] == (K.C_KZG_BADARGS, False) and got[65] != (K.C_KZG_OK, True)
    # and the other way round: group 1 flagged, groups 64 and 65 live -- a kernel that read its flag at blockIdx.y would zero group 65's slot
    items = list(library_cells[mode][200:266])
    items[1] = (items[1][0], 128) + items[1][2:]
    groups = [[it] for it in items]
    with _mode(K, gpu_setup, mode):
        got, _ = _same_as_the_synchronous_call(K, gpu_setup, verifier, groups, "66 x 1, a flag in the first chunk")
        alone = [_rc(K, gpu_setup, grp) for grp in groups]
    assert got == alone
    assert got == [(K.C_KZG_OK, True)] + [(K.C_KZG_BADARGS, False)] + [(K.C_KZG_OK, True)] * 64


@pytest.mark.parametrize("sizes", [[100, 156, 0, 1], [3, 700, 0, 321, 1]], ids=["n257", "n1025"])
@pytest.mark.parametrize("mode", MODES)
def test_uneven_groups_across_the_workgroups_and_the_scan_chunk(K, gpu_setup, verifier, library_cells, mode, sizes):
    """257: a group boundary inside a 256-lane workgroup and a group that spans two; 1025: a group that straddles the scan's 1024-item
    chunk, and the last group alone behind it"""
    groups = _cut(library_cells[mode], sizes)
    with _mode(K, gpu_setup, mode):
        got, _ = _same_as_the_synchronous_call(K, gpu_setup, verifier, groups, sizes)
        assert got == [(K.C_KZG_OK, True)] * len(sizes)
        # the last item's proof swapped for the first one's: the last group alone answers false
        groups[-1] = [groups[-1][0][:3] + (groups[0][0][3],)]
        got, _ = _same_as_the_synchronous_call(K, gpu_setup, verifier, groups, sizes)
        assert got == [(K.C_KZG_OK, True)] * (len(sizes) - 1) + [(K.C_KZG_OK, False)]


# ---- de-duplication ------------------------------------------------------------------------------------------------------------------------------

def _dedup_groups(items):
    """blob 0's cells in three groups, beside blob 1's: one commitment repeated inside a group, and the same one in several groups"""
    a, b = items[:128], items[128:256]
    return [a[:10] + b[:3] + a[10:12], [], b[3:5] + a[12:20] + [a[12]], a[20:23], b[5:6] + b[5:6]]


@pytest.mark.parametrize("mode", MODES)
def test_a_commitment_repeated_inside_a_group_and_across_groups(K, gpu_setup, verifier, library_cells, mode):
    groups = _dedup_groups(library_cells[mode])
    assert _rows(groups) == [2, 0, 2, 1, 1] and [len(g) for g in groups] == [15, 0, 11, 3, 2]
    with _mode(K, gpu_setup, mode):
        got, _ = _same_as_the_synchronous_call(K, gpu_setup, verifier, groups, "dedup")     # (partials equal, and m == the rows' total)
    assert got == [(K.C_KZG_OK, True)] * 5


def _plan(groups):
    """plan_groups (cell_groups_plan.h) restated: rows, row_base, bad words, the concatenated distinct commitments, first_item, the row
    and column lists as sets, and the slice table of the groups that are not dead"""
    n = sum(len(grp) for grp in groups)
    p = {"rows": [], "row_base": [0], "bad_words": [], "distinct": [], "first_item": [], "row_sets": [], "col_sets": [], "slices": [],
         "slice_off": [0]}
    lo = 0
    for j, grp in enumerate(groups):
        dead = any(i[1] >= 128 for i in grp)
        p["bad_words"].append(1 if dead else 0)
        seen, cols = {}, [set() for _ in range(128)]
        if not dead:
            for t, it in enumerate(grp):
                if it[0] not in seen:
                    seen[it[0]] = len(seen)
                    p["distinct"].append(it[0])
                    p["first_item"].append(lo + t)
                    p["row_sets"].append(set())
                p["rows"].append(seen[it[0]])
                p["row_sets"][p["row_base"][-1] + seen[it[0]]].add(lo + t)
                cols[it[1]].add(lo + t)
        else:
            p["rows"] += [0] * len(grp)
        p["col_sets"] += cols
        for s, (first, count) in enumerate([(lo, len(grp)), (lo, len(grp)), (p["row_base"][-1], len(seen))]):
            if not dead:
                p["slices"] += [(j, s, first + at, min(64, count - at)) for at in range(0, count, 64)]
            p["slice_off"].append(len(p["slices"]))
        p["row_base"].append(p["row_base"][-1] + len(seen))
        lo += len(grp)
    p["m"] = p["row_base"][-1]
    p["distinct"] = b"".join(p["distinct"]) + (bytes([0xc0]) + bytes(47)) * (n - p["m"])
    return p


def _sets(perm, off):
    return [set(perm[off[q]:off[q + 1]]) for q in range(len(off) - 1)]


@pytest.mark.parametrize("hash_mask", [0, 0xffffffff], ids=["one_chain", "spread"])
def test_segmented_grouping_hook_against_the_plan_restated(K, library_cells, hash_mask):
    """every key on one probe chain (hash_mask 0) and spread; the order inside a row or column list is undefined: compared as sets"""
    items = library_cells[S.MODE_REFERENCE]
    bad = lambda it: (it[0], 128 + it[1]) + it[2:]
    cases = {"dedup": _dedup_groups(items),
             "boundaries": _cut(items, BOUNDARY_SIZES),
             "n257": _cut(items, [100, 156, 0, 1]),
             "n1025": _cut(items, [3, 700, 0, 321, 1]),
             "bad index first, inside and last": [[bad(items[0]), items[1]], items[2:70], [items[70], bad(items[71])], items[72:80], [bad(items[80])]]}
    for name, groups in cases.items():
        flat = [it for grp in groups for it in grp]
        d = _Dev(flat)
        got = K.cell_group_segmented_device(d.dc.data_ptr(), d.di.data_ptr(), d.n, [len(grp) for grp in groups], 0x1234, hash_mask)
        want = _plan(groups)
        for key in ("m", "rows", "row_base", "bad_words", "distinct", "first_item", "slice_off", "slices"):
            assert got[key] == want[key], (name, key)
        live = sum(len(grp) for grp, dead in zip(groups, want["bad_words"]) if not dead)
        assert got["row_off"][0] == 0 and got["row_off"][-1] == live and got["col_off"][0] == 0 and got["col_off"][-1] == live, name
        assert _sets(got["perm_row"], got["row_off"]) == want["row_sets"], name
        assert _sets(got["perm_col"], got["col_off"]) == want["col_sets"], name
        assert all(x == 0xffffffff for x in got["perm_row"][live:] + got["perm_col"][live:]), name


# ---- bad groups among good ones ----------------------------------------------------------------------------------------------------------------

def _bad_groups(items, mode):
    c, k, cell, proof = items[40]
    good = [items[0:5], items[130:140], items[300:301], items[5:30], items[500:503], items[30:33]]
    return [good[0],
            [items[33], (c, 128, cell, proof), items[34]],                                    # 1: an index >= 128
            good[1],
            [items[35], (c, k, cell, _x_off_the_curve())],                                    # 3: a proof off the curve
            good[2],
            [(ORDER3, k, cell, proof), items[36], items[37]],                                 # 5: a commitment outside the subgroup
            good[3],
            [items[38], items[39], (c, k, cell[:64] + S.to_bytes(R, mode) + cell[96:], proof)],   # 7: a cell element >= r
            good[4],
            [items[41], (items[42][0], items[42][1], items[43][2], items[42][3]), items[44]],     # 9: a tampered cell
            good[5]]


@pytest.mark.parametrize("mode", MODES)
def test_bad_groups_among_good_ones(K, gpu_setup, verifier, library_cells, mode):
    groups = _bad_groups(library_cells[mode], mode)
    code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    with _mode(K, gpu_setup, mode):
        got, partials = _same_as_the_synchronous_call(K, gpu_setup, verifier, groups, "bad groups")
    want = [(K.C_KZG_OK, True)] * 11
    want[1], want[3], want[5], want[7], want[9] = (K.C_KZG_BADARGS, False), (code, False), (code, False), (code, False), (K.C_KZG_OK, False)
    assert got == want and verifier.pending() == 0
    assert [p == ZERO for p in partials] == [j in (1, 3, 5, 7) for j in range(11)]   # (a tampered group was summed: its partials say what)


@pytest.mark.parametrize("mode", MODES)
def test_a_bad_index_first_and_last_leaves_nothing_stale_behind(K, gpu_setup, library_cells, mode):
    """a fresh verifier whose FIRST call has a bad-index group in front and one at the very end (nothing behind r has ever run on its
    buffers), then an honest call of other sizes, back to back without a wait in between, then both again"""
    items = library_cells[mode]
    bad = lambda it: (it[0], 1 << 40) + it[2:]
    first = [[items[0], bad(items[1])], items[2:70], items[70:75], [bad(items[75])]]
    honest = _cut(items[128:], [3, 66, 0, 7])
    v = K.CellVerifier(gpu_setup, 160, 8)
    try:
        with _mode(K, gpu_setup, mode):
            d1, d2 = _Dev([it for grp in first for it in grp]), _Dev([it for grp in honest for it in grp])
            calls = [v.enqueue_groups(*d.ptrs(), d.n, [len(grp) for grp in groups]) for d, groups in ((d1, first), (d2, honest)) * 2]
            v.wait()
            want1, want2 = [K.verify_cell_kzg_proof_groups_device(*d.ptrs(), d.n, [len(grp) for grp in groups], gpu_setup)
                            for d, groups in ((d1, first), (d2, honest))]
            p1, p2 = K.cell_verify_groups_partials(first, gpu_setup), K.cell_verify_groups_partials(honest, gpu_setup)
        assert want1 == [(K.C_KZG_BADARGS, False), (K.C_KZG_OK, True), (K.C_KZG_OK, True), (K.C_KZG_BADARGS, False)]
        assert want2 == [(K.C_KZG_OK, True)] * 4
        assert [c.answers() for c in calls] == [want1, want2] * 2
        assert [c.partials() for c in calls] == [p1, p2] * 2
        assert [(c.result.rc, c.result.ok, c.result.first_bad, c.result.m) for c in calls] == [(0, 0, 0, 2), (0, 1, NONE_BAD, 3)] * 2
    finally:
        v.free()


# ---- shell behaviour -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_one_group_answers_as_the_batch_verifier(K, gpu_setup, verifier, library_cells, mode):
    items = library_cells[mode][60:200]
    with _mode(K, gpu_setup, mode):
        for batch, want_ok in ((items, True), (items[:-1] + [items[-1][:3] + (items[0][3],)], False)):
            d = _Dev(batch)
            grouped = verifier.enqueue_groups(*d.ptrs(), d.n, [d.n])
            plain = verifier.enqueue(*d.ptrs(), d.n)
            verifier.wait()
            assert grouped.answers() == [(plain.rc, bool(plain.ok))] == [(K.C_KZG_OK, want_ok)]
            assert grouped.partials() == [bytes(plain.partials)] and grouped.result.m == plain.m == 2


def test_enqueue_returns_without_waiting_and_the_answers_are_in_stream_order(K, gpu_setup, verifier, library_cells):
    """long work queued ahead on the caller's stream: enqueue_groups returns with the result pending and the stream busy. Work
    enqueued BEHIND the call sees state == 1: a proof overwritten on the stream after the first enqueue does not reach it, and reaches
    the second"""
    import torch
    groups = _cut(library_cells[S.MODE_REFERENCE], [20, 0, 30, 5])
    sizes = [len(grp) for grp in groups]
    d = _Dev([it for grp in groups for it in grp])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _mode(K, gpu_setup, S.MODE_REFERENCE):
        _long_work(torch, st)
        first = verifier.enqueue_groups(*d.ptrs(), d.n, sizes, st.cuda_stream)
        state, pending, drained = first.result.state, verifier.pending(), st.query()
        with torch.cuda.stream(st):
            d.dp[48 * 27:48 * 28] = d.dp[48 * 3:48 * 4].clone()   # ordered behind the first call: enqueue joins its end into the stream
        second = verifier.enqueue_groups(*d.ptrs(), d.n, sizes, st.cuda_stream)
        assert (state, pending, drained) == (0, 1, False)
        st.synchronize()                                          # the stream was ordered behind both calls: no wait on the verifier
        assert (first.result.state, second.result.state) == (1, 1)
        verifier.wait()
    assert first.answers() == [(0, True)] * 4 and second.answers() == [(0, True), (0, True), (0, False), (0, True)]
    assert (second.result.ok, second.result.first_bad) == (0, 2)


def test_depth_plus_two_calls_back_to_back_batch_and_grouped_in_turn(K, gpu_setup, verifier, library_cells):
    items = library_cells[S.MODE_REFERENCE]
    groups = _cut(items, [40, 1, 0, 70])
    flat = [it for grp in groups for it in grp]
    good, bad = _Dev(flat), _Dev(flat[:50] + [flat[50][:3] + (flat[51][3],)] + flat[51:])      # item 50 is of group 3
    sizes = [len(grp) for grp in groups]
    calls, seen = [], []
    with _mode(K, gpu_setup, S.MODE_REFERENCE):
        for q in range(K.VERIFIER_DEPTH + 2):
            d = bad if q % 3 == 2 else good
            calls.append(verifier.enqueue_groups(*d.ptrs(), d.n, sizes) if q & 1 else verifier.enqueue(*d.ptrs(), d.n))
            seen.append(verifier.pending())
        verifier.wait()
    assert max(seen) <= K.VERIFIER_DEPTH and min(seen) >= 0, seen
    for q, c in enumerate(calls):
        ok = q % 3 != 2
        if q & 1:
            assert c.answers() == [(0, True)] * 3 + [(0, ok)] and (c.result.state, c.result.rc, c.result.ok) == (1, 0, int(ok)), q
        else:
            assert (c.state, c.rc, c.ok) == (1, 0, int(ok)), q


def test_two_verifiers_on_two_streams_beside_a_synchronous_grouped_call(K, gpu_setup, verifier, library_cells):
    import torch
    mode = S.MODE_REFERENCE
    items = library_cells[mode]
    gpu_setup.reserve(8, caller_streams=2)
    second = K.CellVerifier(gpu_setup, 300, 4)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        g1, g3, small = _cut(items, [100, 156, 0, 1]), _cut(items[300:], [1, 200, 56]), _cut(items[900:], [10, 20])
        g2 = _cut(items[600:700] + [items[700][:3] + (items[701][3],)] + items[701:857], [90, 20, 147])     # the tampered item is of group 1
        d1, d2, d3, ds = [_Dev([it for grp in g for it in grp]) for g in (g1, g2, g3, small)]
        with _mode(K, gpu_setup, mode):
            r1 = verifier.enqueue_groups(*d1.ptrs(), d1.n, [len(x) for x in g1], s1.cuda_stream)
            sync = K.verify_cell_kzg_proof_groups_device(*ds.ptrs(), ds.n, [10, 20], gpu_setup)
            r2 = second.enqueue_groups(*d2.ptrs(), d2.n, [len(x) for x in g2], s2.cuda_stream)
            r3 = verifier.enqueue_groups(*d3.ptrs(), d3.n, [len(x) for x in g3], s1.cuda_stream)
            verifier.wait()
            second.wait()
        assert sync == [(0, True)] * 2
        assert r1.answers() == [(0, True)] * 4 and r2.answers() == [(0, True), (0, False), (0, True)] and r3.answers() == [(0, True)] * 3
        assert [(r.result.state, r.result.rc, r.result.ok, r.result.m) for r in (r1, r2, r3)] == [(1, 0, 1, 4), (1, 0, 0, 5), (1, 0, 1, 5)]
        torch.cuda.synchronize()
    finally:
        second.free()


def test_completions_on_the_spot(K, gpu_setup, verifier, library_cells):
    import ctypes as C
    items = library_cells[S.MODE_REFERENCE][:12]
    d = _Dev(items)
    l = K.lib()

    def refused(v, ptrs, n, offsets, g, ok=True, rc=True):
        res = K.CellVerifyResult()
        okb, rcb, part = (C.c_uint8 * 4)(7, 7, 7, 7), (C.c_int32 * 4)(-5, -5, -5, -5), C.create_string_buffer(b"\x11" * (4 * len(ZERO)), 4 * len(ZERO))
        off = (C.c_uint64 * len(offsets))(*offsets) if offsets is not None else None
        got = l.lwkzg_cell_verifier_enqueue_groups(v.h, C.byref(res), okb if ok else None, rcb if rc else None, part, *ptrs, n, off, g, None)
        assert list(okb) == [7] * 4 and list(rcb) == [-5] * 4 and part.raw == b"\x11" * (4 * len(ZERO))      # nothing but *result is written
        assert v.pending() == 0
        return got, (res.state, res.rc, res.ok, res.first_bad, res.m)

    done = (K.C_KZG_BADARGS, (1, K.C_KZG_BADARGS, 0, NONE_BAD, 0))
    # the grouped call's own call-level errors: bad offsets, g == 0 with n > 0, a NULL item array, NULL ok_out / rc_out / offsets
    for off in ([1, 5, 12], [0, 5, 11], [0, 7, 5], [0, 13, 12]):
        assert refused(verifier, d.ptrs(), 12, off, 2) == done, off
    assert refused(verifier, d.ptrs(), 12, [0], 0) == done
    assert refused(verifier, d.ptrs(), 12, None, 2) == done
    for missing in range(4):
        ptrs = list(d.ptrs())
        ptrs[missing] = None
        assert refused(verifier, ptrs, 12, [0, 5, 12], 2) == done, missing
    assert refused(verifier, d.ptrs(), 12, [0, 5, 12], 2, ok=False) == done and refused(verifier, d.ptrs(), 12, [0, 5, 12], 2, rc=False) == done
    # n above max_cells, g above max_groups, a verifier from lwkzg_cell_verifier_new
    small, plain = K.CellVerifier(gpu_setup, 8, 2), K.CellVerifier(gpu_setup, 64)
    try:
        assert refused(small, d.ptrs(), 9, [0, 4, 9], 2) == done
        assert refused(small, d.ptrs(), 8, [0, 4, 6, 8], 3) == done
        assert refused(plain, d.ptrs(), 12, [0, 5, 12], 2) == done
        with pytest.raises(K.KzgError) as e:
            K.CellVerifier(gpu_setup, 8, (1 << 30) + 1)
        assert e.value.rc == K.C_KZG_BADARGS
        # g == n == 0: OK, ok = 1, nothing written; empty groups alone: (OK, 1) and zero partials for each, on the spot as well
        assert refused(verifier, (None,) * 4, 0, None, 0) == (K.C_KZG_OK, (1, K.C_KZG_OK, 1, NONE_BAD, 0))
        ans = verifier.enqueue_groups(None, None, None, None, 0, [0, 0, 0])
        assert ans.result.state == 1 and ans.answers() == [(K.C_KZG_OK, True)] * 3 and ans.partials() == [ZERO] * 3
        with _mode(K, gpu_setup, S.MODE_REFERENCE):       # and the small verifier works: a call that fills it, as a batch and in groups
            ans, res = small.enqueue_groups(*d.ptrs(), 8, [3, 5]), small.enqueue(*d.ptrs(), 8)
            small.wait()
            assert ans.answers() == [(0, True)] * 2 and (res.state, res.rc, res.ok) == (1, 0, 1)
    finally:
        small.free()
        plain.free()


def test_setup_freed_under_a_verifier(K, library_cells):
    """free_trusted_setup waits for the grouped call in flight; the verifier then refuses, and is still freed cleanly"""
    groups = _cut(library_cells[S.MODE_REFERENCE], [10, 0, 30])
    d = _Dev([it for grp in groups for it in grp])
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    ts.set_mode(K.MODE_REFERENCE)
    v = K.CellVerifier(ts, 64, 4)
    ans = v.enqueue_groups(*d.ptrs(), d.n, [10, 0, 30])
    ts.free()
    assert (ans.result.state, ans.result.rc, ans.result.ok, ans.result.first_bad) == (1, 0, 1, NONE_BAD)
    assert ans.answers() == [(0, True)] * 3
    with pytest.raises(K.KzgError) as e:
        v.enqueue_groups(*d.ptrs(), d.n, [10, 0, 30])
    assert e.value.rc == K.C_KZG_BADARGS and e.value.result.state == 1
    v.free()
    assert v.pending() == -1


@pytest.mark.parametrize("mode", MODES)
def test_both_engines(K, engine_setup, library_cells, mode):
    items = library_cells[mode]
    v = K.CellVerifier(engine_setup, 400, 16)
    try:
        with _mode(K, engine_setup, mode):
            got, _ = _same_as_the_synchronous_call(K, engine_setup, v, _cut(items, BOUNDARY_SIZES), "engines")
            assert got == [(K.C_KZG_OK, True)] * len(BOUNDARY_SIZES)
            got, _ = _same_as_the_synchronous_call(K, engine_setup, v, _bad_groups(items, mode), "engines, bad groups")
            assert [a == (K.C_KZG_OK, True) for a in got] == [j % 2 == 0 for j in range(11)]
    finally:
        v.free()
