"""CPU: the special blobs of tests/flag_cases.py are what they claim to be, by the reference alone. From the setup's secret every lane
sum and every partial sum of a lane is an integer mod r: exactly the intended lanes coincide, the collision sits where the kind says
(inside a lane's chain of additions: the accumulation raises the flag; between two finished lane sums: the fold does), and nothing
else coincides. On the monomial setup and on its Lagrange form, and the positions the GPU tests rely on at n = 1023 and n = 1024."""
import pytest

import flag_cases as F

R = F.R


def _by_kind(lagrange):
    """one special blob of every kind out of full_chunk_batch's layout (the scalars alone: no batch is built)"""
    out = {}
    for index, kind in F.special_layout(1024, 1):
        out.setdefault(kind, F.special_scalars(kind, 1000 + index, lagrange))
    assert sorted(out) == sorted(F.KINDS)
    return out


def _check(kind, ss, lagrange, all_lanes_width=None):
    """the claims of `kind` about the scalars ss. The lanes the construction touches are walked on every table width; all_lanes_width: ALL
    256 chains on that width too (the random lanes: no collision anywhere)."""
    assert len(ss) == F.N and all(0 <= s < R for s in ss)
    sums = F.lane_sums(ss, lagrange)
    pairs = F.coinciding_lanes(sums)
    live = [t for t in range(F.LANES) if sums[t]]
    if kind == "zero":
        assert not any(ss) and not live
        return
    if kind == "one_scalar":
        assert sum(1 for s in ss if s) == 1 and len(live) == 1 and not pairs
        assert not F.lane_chain_collisions(ss, 13, live, lagrange)
        return
    want_pair, touched = [], []
    if kind.startswith("fold") or kind == "acc_and_fold":
        a, b, others = F.FOLD_PAIRS[0 if kind == "acc_and_fold" else int(kind[4])]
        lo, hi = min(a, b), max(a, b)
        want_pair = [(lo, hi, -1 if kind.endswith("opp") else 1)]
        touched += [a, b]
        # each of the two lanes holds ONE scalar: its chain is the digits of that scalar and its sum is final before the fold reads it
        assert [i for i in range(F.N) if i % 256 in (a, b) and ss[i]] == sorted((a, b))
        if not (others or kind == "acc_and_fold"):
            assert live == sorted((a, b))
    assert pairs == want_pair, (kind, pairs)          # exactly the intended pair is equal or opposite; no other two lanes coincide
    acc_lane = None
    if kind in F.ACC_KINDS:
        # the lane whose first scalar is followed by seven zeros and a one-digit scalar
        cands = [t for t in range(F.LANES) if ss[t] and not any(ss[t + 256 * m] for m in range(1, 8)) and 0 < ss[t + 2048] < 512]
        cands = [t for t in cands if t not in touched]
        assert len(cands) == 1, (kind, cands)
        acc_lane = cands[0]
        touched.append(acc_lane)
    for c in F.WIDTHS:
        hits = F.lane_chain_collisions(ss, c, range(F.LANES) if c == all_lanes_width else touched, lagrange)
        if acc_lane is None:
            assert not hits, (kind, c, hits)          # no partial sum inside a lane equals +- the next row: the flag comes from the fold
        else:
            # inside the lane's chain: its accumulator after ALL digits of the first scalar against the one row of scalar t + 2048
            sign = 1 if kind == "acc_eq" else -1
            assert hits == [(acc_lane, acc_lane + 2048, 0, sign)], (kind, c, hits)


@pytest.mark.parametrize("lagrange", [False, True], ids=["monomial", "lagrange"])
def test_every_special_blob_of_the_full_chunk(lagrange):
    """all forty special blobs of the batch the GPU tests run: the lanes their constructions touch on every table width, all 256 lanes on
    the default one"""
    for index, kind in F.special_layout(1024, 1):
        _check(kind, F.special_scalars(kind, 1000 + index, lagrange), lagrange, all_lanes_width=13)


def test_the_pair_survives_two_workgroups_per_blob():
    """the fused commit-and-prove call spreads a blob over two workgroups (512 lanes: lane t owns t, t + 512, ...): the fold pairs and
    the colliding chain are among the first 256 lanes -- one fold wave's share -- there too"""
    for kind, ss in _by_kind(False).items():
        if kind in ("zero", "one_scalar"):
            continue
        sums = F.lane_sums(ss, lanes_per_blob=512)
        pairs = F.coinciding_lanes(sums)
        hits = F.lane_chain_collisions(ss, 13, range(512), lanes_per_blob=512)
        if kind in F.ACC_KINDS:
            assert len(hits) == 1 and hits[0][0] < 256 and hits[0][1] == hits[0][0] + 2048, (kind, hits)
        else:
            assert not hits, (kind, hits)
        if kind.startswith("fold") or kind == "acc_and_fold":
            a, b, _ = F.FOLD_PAIRS[0 if kind == "acc_and_fold" else int(kind[4])]
            assert pairs == [(min(a, b), max(a, b), -1 if kind.endswith("opp") else 1)], (kind, pairs)
        else:
            assert not pairs


def test_the_constructions_that_moved_here_collide_where_they_say():
    """fold_collision_scalars (tests/commit_tail_worker.py's 512-blob batch) and one_colliding_lane_blob (tests/test_gpu_parity.py)"""
    import random
    for blob in range(8):
        ss = F.fold_collision_scalars(blob)
        a, b, _ = F.FOLD_PAIRS[(blob // 2) % 4]
        assert F.coinciding_lanes(F.lane_sums(ss)) == [(min(a, b), max(a, b), -1 if blob % 2 else 1)]
        assert not F.lane_chain_collisions(ss, 14, (a, b))
    for c in (10, 16):
        for negate in (False, True):
            ss = F.one_colliding_lane_blob(random.Random(c), c, negate)
            hits = F.lane_chain_collisions(ss, c, range(F.LANES))
            assert len(hits) == 1 and hits[0][1] == hits[0][0] + 2048 and hits[0][2:] == (0, -1 if negate else 1), hits


@pytest.mark.parametrize("n", [1023, 1024, 1536, 2049])
def test_positions(n):
    layout = F.special_layout(n, 1)
    at = dict(layout)
    assert len(at) == F.N_SPECIAL == len(layout)
    want = {0, 1, 255, 256, 511, 512, 767, n - 2, n - 1} | {i for i in (1023, 1024, 2047, 2048) if i < n}
    assert want <= set(at)
    # one row of the second pass (256 rows of workgroups, blob = row + 256 m) finds four blobs the ACCUMULATION flagged
    run = [i for i in at if i % 256 == F.ROW_RUN[0] % 256]
    assert run == list(F.ROW_RUN) and all(at[i] in F.ACC_KINDS for i in run)
    # every kind is there, and the last quarter of a full chunk holds accumulation and fold flags both
    assert set(at.values()) == set(F.KINDS)
    assert any(at[i] in F.ACC_KINDS for i in at if 768 <= i < 1023) and any(at[i].startswith("fold") for i in at if 768 <= i < 1023)
    # honest blobs between flagged ones: three or more, but for the adjacent pairs at the boundaries above
    idx = sorted(at)
    close = [(i, j) for i, j in zip(idx, idx[1:]) if j - i <= 3]
    assert all(j - i == 1 and (i in want and j in want) for i, j in close), close
    assert len(F.honest_sample(n, [F.Special(i, k, None) for i, k in layout])) > 17 + 40


def test_batch_bytes():
    """the batch: honest blobs are B.synthetic_blob's, special blobs carry their scalars in the mode's byte order, all below r"""
    import blobs as B
    for lagrange in (False, True):
        data, specials = F.full_chunk_batch(1023, 2, lagrange)
        assert len(data) == 1023 * B.BYTES_PER_BLOB and [(s.index, s.kind) for s in specials] == F.special_layout(1023, 2)
        for s in specials:
            assert F.blob_scalars_at(data, s.index, lagrange) == s.scalars
        for i in F.honest_sample(1023, specials)[:5]:
            assert data[i * B.BYTES_PER_BLOB:(i + 1) * B.BYTES_PER_BLOB] == B.synthetic_blob(2000 + i, big_endian=not lagrange)
