"""GPU: the grouping kernels of the asynchronous cell verifier (lambdaworks_kzg_amd/csrc/cell_group.hip) through
the test hook lwkzg_cell_group_device. No valid points are needed: the inputs are arbitrary 48-byte strings and indices, held against
a Python dict model of group_items (cells_verify_api.hip) -- rows, m, the distinct strings and their infinity padding, first_item,
row_off, col_off and bad_index exactly; the groups of perm_row / perm_col as sets, since the order inside a group is the atomics'."""
import random

import pytest

pytestmark = pytest.mark.gpu

INF = bytes([0xc0]) + bytes(47)
NONE_BAD = 0xffffffff
SEED = 0x5eed5eed5eed5eed


def _model(strings, idx):
    seen, rows, distinct, first_item = {}, [], [], []
    for i, s in enumerate(strings):
        if s not in seen:
            seen[s] = len(distinct)
            distinct.append(s)
            first_item.append(i)
        rows.append(seen[s])
    m, n = len(distinct), len(strings)
    by_row = [set() for _ in range(m)]
    by_col = [set() for _ in range(128)]
    for i, (r, k) in enumerate(zip(rows, idx)):
        by_row[r].add(i)
        if k < 128:
            by_col[k].add(i)
    bad = [i for i, k in enumerate(idx) if k >= 128]
    return {"rows": rows, "m": m, "distinct": b"".join(distinct) + INF * (n - m), "first_item": first_item, "by_row": by_row,
            "by_col": by_col, "bad_index": bad[0] if bad else NONE_BAD}


def _run(K, strings, idx, seed=SEED, hash_mask=0xffffffff):
    import torch
    n = len(strings)
    dc = torch.frombuffer(bytearray(b"".join(strings)), dtype=torch.uint8).cuda()
    di = torch.tensor([k - (1 << 64) if k >= 1 << 63 else k for k in idx], dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    return K.cell_group_device(dc.data_ptr(), di.data_ptr(), n, seed, hash_mask)


def _groups(perm, off):
    out = []
    for g in range(len(off) - 1):
        members = perm[off[g]:off[g + 1]]
        assert len(set(members)) == len(members), g
        out.append(set(members))
    return out


def _check(K, strings, idx, **kw):
    got, want = _run(K, strings, idx, **kw), _model(strings, idx)
    n = len(strings)
    assert got["m"] == want["m"] and got["bad_index"] == want["bad_index"]
    assert got["rows"] == want["rows"] and got["first_item"] == want["first_item"] and got["distinct"] == want["distinct"]
    assert got["row_off"] == [0] + [sum(len(g) for g in want["by_row"][:j + 1]) for j in range(want["m"])] and got["row_off"][-1] == n
    assert got["col_off"] == [0] + [sum(len(g) for g in want["by_col"][:k + 1]) for k in range(128)]
    assert _groups(got["perm_row"], got["row_off"]) == want["by_row"]
    assert _groups(got["perm_col"], got["col_off"]) == want["by_col"]
    return got


def _strings(rnd, n, distinct):
    pool = [rnd.randbytes(48) for _ in range(distinct)]
    return [pool[rnd.randrange(distinct)] for _ in range(n)] if distinct < n else pool


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1025, 4097])
def test_sizes_at_the_workgroup_and_chunk_edges(K, n):
    """256 lanes per workgroup in the per-item kernels, 1024 items per chunk of the single-workgroup scans, and more than four chunks;
    all equal, all distinct, and 37 (or n, if fewer) distinct strings"""
    rnd = random.Random(4100 + n)
    for distinct in (1, n, min(37, n)):
        _check(K, _strings(rnd, n, distinct), [rnd.randrange(128) for _ in range(n)])


def test_thirty_seven_distinct_among_three_hundred(K):
    rnd = random.Random(4137)
    got = _check(K, _strings(rnd, 300, 37), [rnd.randrange(128) for _ in range(300)])
    assert got["m"] == 37


def test_strings_that_differ_in_four_bytes_only(K):
    """equal except in the last four bytes, equal except in the first byte: the compare reads all 48, the hash mixes all 48"""
    rnd = random.Random(4148)
    base = rnd.randbytes(48)
    n = 300
    idx = [rnd.randrange(128) for _ in range(n)]
    tails = [base[:44] + (i % 150).to_bytes(4, "little") for i in range(n)]
    assert _check(K, tails, idx)["m"] == 150
    heads = [bytes([i % 200]) + base[1:] for i in range(n)]
    assert _check(K, heads, idx)["m"] == 200


@pytest.mark.parametrize("hash_mask", [0, 1])
def test_every_key_on_one_probe_chain_and_on_two(K, hash_mask):
    rnd = random.Random(4200 + hash_mask)
    for distinct in (300, 37):
        _check(K, _strings(rnd, 300, distinct), [rnd.randrange(128) for _ in range(300)], hash_mask=hash_mask)


def test_two_seeds_give_the_same_outputs(K):
    rnd = random.Random(4300)
    strings, idx = _strings(rnd, 1025, 200), [rnd.randrange(128) for _ in range(1025)]
    a, b = _check(K, strings, idx, seed=1), _check(K, strings, idx, seed=0xfedcba9876543210)
    for key in ("rows", "m", "distinct", "first_item", "row_off", "col_off", "bad_index"):
        assert a[key] == b[key], key


def test_column_extremes(K):
    rnd = random.Random(4400)
    strings = _strings(rnd, 1025, 9)
    _check(K, strings, [77] * 1025)                       # all one column
    _check(K, strings, [i % 128 for i in range(1025)])    # all 128 columns
    _check(K, strings, [127 - (i % 128) for i in range(1025)])


@pytest.mark.parametrize("where", [3, 1000])
@pytest.mark.parametrize("value", [128, 1 << 63])
def test_an_index_out_of_range_is_reported_and_is_nobodys_subscript(K, where, value):
    """bad_index is the LOWEST such item; such items are in no column, every other output is as always"""
    rnd = random.Random(4500 + where)
    strings = _strings(rnd, 1025, 64)
    idx = [rnd.randrange(128) for _ in range(1025)]
    idx[where] = value
    assert _check(K, strings, idx)["bad_index"] == where
    idx[1010] = (1 << 64) - 1                            # a second one further back does not move it ...
    assert _check(K, strings, idx)["bad_index"] == where
    idx[1] = 200                                         # ... a lower one does
    assert _check(K, strings, idx)["bad_index"] == 1
