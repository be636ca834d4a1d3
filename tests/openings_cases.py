"""Openings (C, z, y, pi) for the batch verification tests (test_gpu_verify_openings.py, test_gpu_verify_openings_async.py): a pool
of honest openings per mode, computed once -- 65 synthetic blobs opened at three points each --, larger batches drawn from it by
repetition (repeated items are legal), every kind of defect put at random places, and the truth per item: the single
verify_kzg_proof call, remembered per distinct item."""
import ctypes as C
import random

import blobs as B
from conftest import R

INF = bytes([0xc0]) + bytes(47)
INF_STRAY = bytes([0xc0]) + bytes(46) + b"\x01"   # the infinity flag with a stray bit: accepted, canonical form INF
N_BLOBS, POINTS = 65, 3

# defects that leave every item validly encoded (the verdict decides) / that make verify_kzg_proof refuse the item (the code decides)
VERDICT_KINDS = ["swap_proof", "swap_commitment", "y_plus_one", "inf_stray", "zero_poly", "pi_inf"]
CODE_KINDS = ["bad_c", "bad_pi", "z_ge_r", "y_ge_r"]

_pools = {}
_truth = {}


def order_of(K, mode):
    return "little" if mode == K.MODE_CKZG else "big"


def mode_code(K, mode):
    return K.C_KZG_ERROR if mode == K.MODE_REFERENCE else K.C_KZG_BADARGS


class Mode:
    """the settings answer in `mode` inside the block"""

    def __init__(self, ts, mode):
        self.ts, self.mode = ts, mode

    def __enter__(self):
        self.ts.set_mode(self.mode)

    def __exit__(self, *exc):
        self.ts.set_mode(-1)


def pool(K, ts, mode):
    """[(C, z, y, pi)] * 195, honest, in `mode` (call inside Mode(ts, mode))"""
    if mode not in _pools:
        rnd = random.Random(5100 + mode)
        order = order_of(K, mode)
        blobs = [B.synthetic_blob(52000 + 100 * mode + i, big_endian=mode != K.MODE_CKZG) for i in range(N_BLOBS)]
        cms = K.blob_to_kzg_commitment_batch(b"".join(blobs), ts)
        zs = [rnd.randrange(R).to_bytes(32, order) for _ in range(N_BLOBS * POINTS)]
        w = pow(7, (R - 1) // 4096, R)
        zs[4] = pow(w, 77, R).to_bytes(32, order)   # a z on the evaluation domain
        res = K.compute_kzg_proof_batch(b"".join(blobs[i % N_BLOBS] for i in range(len(zs))), b"".join(zs), ts)
        _pools[mode] = [(cms[i % N_BLOBS], zs[i], y, p) for i, (p, y) in enumerate(res)]
    return _pools[mode]


def draw(items, n, seed):
    """n honest items: the pool in order, then repeated at random"""
    rnd = random.Random(seed)
    return [items[i] if i < len(items) else items[rnd.randrange(len(items))] for i in range(n)]


def tamper_y(K, mode, item):
    c, z, y, p = item
    order = order_of(K, mode)
    return (c, z, ((int.from_bytes(y, order) + 1) % R).to_bytes(32, order), p)


def with_defects(K, mode, items, kinds, seed):
    """a copy of `items` with each kind of defect at one random place (as many kinds as fit beside one honest item); the places"""
    rnd = random.Random(seed)
    items = list(items)
    n, order = len(items), order_of(K, mode)
    places = rnd.sample(range(n), min(len(kinds), max(n - 1, 0)))
    for kind, i in zip(kinds, places):
        c, z, y, p = items[i]
        other = items[(i + 1) % n] if items[(i + 1) % n][0] != c else items[(i + N_BLOBS // 2) % n]
        if kind == "swap_proof":
            p = other[3]
        elif kind == "swap_commitment":
            c = other[0]
        elif kind == "y_plus_one":
            y = tamper_y(K, mode, items[i])[2]
        elif kind == "inf_stray":
            c, y, p = INF_STRAY, bytes(32), INF
        elif kind == "zero_poly":
            c, y, p = INF, bytes(32), INF
        elif kind == "pi_inf":
            p = INF
        elif kind == "bad_c":
            c = bytes([c[0] & 0x7f]) + c[1:]    # compression flag cleared
        elif kind == "bad_pi":
            p = bytes([0xa0]) + bytes(rnd.getrandbits(8) for _ in range(47))
        elif kind == "z_ge_r":
            z = (R + rnd.randrange(1 << 200)).to_bytes(32, order)
        elif kind == "y_ge_r":
            y = R.to_bytes(32, order)
        items[i] = (c, z, y, p)
    return items, sorted(places)


def columns(items):
    """(commitments, zs, ys, proofs), each concatenated"""
    return tuple(b"".join(t[k] for t in items) for k in range(4))


def single(K, item, ts):
    ok = C.c_bool(False)
    rc = K.lib().verify_kzg_proof(C.byref(ok), *item, ts.ref())
    return rc, bool(ok.value)


def truth(K, ts, mode, items, key=None):
    """[(rc, ok)] of the single calls (call inside Mode(ts, mode)); one call per distinct item per setup"""
    memo = _truth.setdefault((key or id(ts), mode), {})
    out = []
    for it in items:
        if it not in memo:
            memo[it] = single(K, it, ts)
        out.append(memo[it])
    return out


def expected(K, mode, singles):
    """(rc, ok, lowest rejected index or None) of the batch call from the single calls' answers"""
    bad = [i for i, (rc, _) in enumerate(singles) if rc != 0]
    if bad:
        assert all(singles[i][0] == mode_code(K, mode) for i in bad)
        return mode_code(K, mode), False, bad[0]
    return 0, all(ok for _, ok in singles), None
