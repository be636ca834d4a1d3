"""GPU: the consensus-specs mode (LWKZG_MODE_ETH) on the EIP-7594 calls -- cells and cell proofs, recovery, cell proof verification.
Expected values: tests/cells_spec.py read in mode 2 (big-endian evaluation form) for one blob, and the library's own c-kzg mode on
byte-reversed inputs for the batches: cells_eth(B) = rev32(cells_ckzg(rev32(B))), the proofs equal (tests/eth_spec.py)."""
import contextlib
import ctypes as C

import pytest

import blobs as B
import cells_spec as S
import eth_spec as E
from conftest import R, SETUP_PATH, tau_closed_form

pytestmark = pytest.mark.gpu

ETH, LAG = 2, 2
BLOB, CELL = B.BYTES_PER_BLOB, 2048
NONE_BAD = 0xffffffff
_cache = {}


def syn(i):
    return B.synthetic_blob(83000 + i)        # big-endian canonical elements


@pytest.fixture(scope="module")
def ts(K):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    t = K.TrustedSetup.from_file(SETUP_PATH)
    t.enable_direct_table_forms(10, LAG)
    yield t
    t.free()


@contextlib.contextmanager
def eth(ts):
    ts.set_mode(ETH)
    try:
        yield ts
    finally:
        ts.set_mode(-1)
        ts.enable_direct_table_forms(10, LAG)


def as_ckzg(ts, fn):
    ts.set_mode(1)
    try:
        return fn()
    finally:
        ts.set_mode(ETH)


def dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def host(t):
    return bytes(t.cpu().numpy().tobytes())


def _made(K, ts, n=9):
    """(blobs, commitments, [(cells, proofs)]) of n blobs in eth mode's bytes through the identity: c-kzg mode on the reversed blobs"""
    if ("made", n) not in _cache:
        blobs = [syn(i) for i in range(n)]
        rdata = E.rev32(b"".join(blobs))
        comms = as_ckzg(ts, lambda: K.blob_to_kzg_commitment_batch(rdata, ts))
        made = as_ckzg(ts, lambda: K.compute_cells_and_kzg_proofs_batch(rdata, ts))
        _cache[("made", n)] = (blobs, comms, [([E.rev32(c) for c in cells], proofs) for cells, proofs in made])
    return _cache[("made", n)]


def test_compute_one_blob_against_the_restatement(K, ts, oracle):
    blob = syn(0)
    with eth(ts):
        cells, proofs = K.compute_cells_and_kzg_proofs(blob, ts)
        poly = S.poly_from_blob(blob, ETH)                       # cells_spec.py: not c-kzg mode -> big-endian; not reference -> evaluations
        assert cells == S.cells_bytes(poly, ETH)
        assert proofs == [tau_closed_form(oracle, S.quotient(poly, k)) for k in range(128)]
        assert b"".join(cells[:64]) == blob                      # the first 64 cells are the blob's own bytes
        blobs, comms, made = _made(K, ts)
        assert (cells, proofs) == made[0]                        # ... which anchors identity (3) for the batches below


def test_compute_batches_and_the_range_rule(K, ts):
    import torch
    with eth(ts):
        blobs, comms, made = _made(K, ts)
        n = len(blobs)
        d_b = dev(b"".join(blobs))
        d_cells = torch.zeros(n * 128 * CELL, dtype=torch.uint8, device="cuda")
        d_proofs = torch.zeros(n * 128 * 48, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        K.compute_cells_and_kzg_proofs_batch_device(d_cells.data_ptr(), None, d_b.data_ptr(), n, ts, None, st.data_ptr())    # cells only
        torch.cuda.synchronize()
        want_cells = b"".join(b"".join(c) for c, _ in made)
        assert host(d_cells) == want_cells and st.tolist() == [0] * n
        d_cells.zero_()
        K.compute_cells_and_kzg_proofs_batch_device(d_cells.data_ptr(), d_proofs.data_ptr(), d_b.data_ptr(), n, ts, None, st.data_ptr())
        torch.cuda.synchronize()
        assert host(d_cells) == want_cells and host(d_proofs) == b"".join(b"".join(p) for _, p in made) and st.tolist() == [0] * n
        # one blob with an element >= r: C_KZG_BADARGS through the host call, its status word alone in the device form
        bad = bytearray(blobs[1])
        bad[32 * 4095:] = b"\xff" + bytes(31)
        data = blobs[0] + bytes(bad) + blobs[2]
        with pytest.raises(K.KzgError) as e:
            K.compute_cells_and_kzg_proofs_batch(data, ts)
        assert e.value.rc == K.C_KZG_BADARGS
        with pytest.raises(K.KzgError) as e:
            K.compute_cells_and_kzg_proofs(bytes(bad), ts)
        assert e.value.rc == K.C_KZG_BADARGS
        st = torch.full((3,), 7, dtype=torch.int32, device="cuda")
        K.compute_cells_and_kzg_proofs_batch_device(d_cells.data_ptr(), d_proofs.data_ptr(), dev(data).data_ptr(), 3, ts, None, st.data_ptr())
        torch.cuda.synchronize()
        assert st.tolist() == [0, K.C_KZG_BADARGS, 0]
        ok_elem = bytearray(blobs[1])
        ok_elem[32 * 4095:] = bytes(31) + b"\xff"
        cells, _ = K.compute_cells_and_kzg_proofs(bytes(ok_elem), ts, proofs=False)
        assert b"".join(cells[:64]) == bytes(ok_elem)


def test_fk20_engine_gives_the_same_bytes(K, ts):
    from lambdaworks_kzg_amd import capi
    with eth(ts):
        blobs, comms, made = _made(K, ts)
        try:
            ts.set_cell_proof_engine(capi.CELL_PROOFS_FK20, 4, 1)
            got = K.compute_cells_and_kzg_proofs_batch(blobs[0] + blobs[1], ts)
            assert got == made[:2]
        finally:
            ts.set_cell_proof_engine(capi.CELL_PROOFS_MSM)


def test_recovery(K, ts):
    import torch
    with eth(ts):
        blobs, comms, made = _made(K, ts)
        cells, proofs = made[0]
        even = list(range(0, 128, 2))
        assert K.recover_cells_and_kzg_proofs(even, [cells[k] for k in even], ts) == made[0]
        idx65 = sorted(set(even) | {1})
        given = [cells[k] for k in idx65]
        assert K.recover_cells_and_kzg_proofs(idx65, given, ts) == made[0]
        # 65 cells with one element changed: no polynomial of degree < 4096 goes through them
        v = (int.from_bytes(given[3][:32], "big") + 1) % R
        changed = given[:3] + [v.to_bytes(32, "big") + given[3][32:]] + given[4:]
        with pytest.raises(K.KzgError) as e:
            K.recover_cells_and_kzg_proofs(idx65, changed, ts)
        assert e.value.rc == K.C_KZG_BADARGS
        # a cell element >= r (big-endian)
        for idx, cs in ((even, [cells[k] for k in even]), (idx65, given)):
            nc = cs[:5] + [cs[5][:64] + b"\xff" + bytes(31) + cs[5][96:]] + cs[6:]
            with pytest.raises(K.KzgError) as e:
                K.recover_cells_and_kzg_proofs(idx, nc, ts)
            assert e.value.rc == K.C_KZG_BADARGS
        # three blobs over two index sets in one call
        odd = list(range(1, 128, 2))
        lists = [even, odd, even]
        got = K.recover_cells_and_kzg_proofs_mixed(lists, [[made[b][0][k] for k in lists[b]] for b in range(3)], ts)
        assert got == made[:3]
        # nine blobs, device-resident
        n = len(blobs)
        d_in = dev(b"".join(made[b][0][k] for b in range(n) for k in even))
        d_cells = torch.zeros(n * 128 * CELL, dtype=torch.uint8, device="cuda")
        d_proofs = torch.zeros(n * 128 * 48, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        K.recover_cells_and_kzg_proofs_batch_device(d_cells.data_ptr(), d_proofs.data_ptr(), even, d_in.data_ptr(), n, ts, None, st.data_ptr())
        torch.cuda.synchronize()
        assert st.tolist() == [0] * n
        assert host(d_cells) == b"".join(b"".join(c) for c, _ in made) and host(d_proofs) == b"".join(b"".join(p) for _, p in made)


def test_cell_verification(K, ts):
    import torch
    from lambdaworks_kzg_amd import capi
    with eth(ts):
        blobs, comms, made = _made(K, ts)
        # one blob's 128 cells, then 3 cells of a second blob, then the first commitment again
        items = [(comms[0], k, made[0][0][k], made[0][1][k]) for k in range(128)]
        items += [(comms[1], k, made[1][0][k], made[1][1][k]) for k in (5, 64, 127)]
        items += [(comms[0], 9, made[0][0][9], made[0][1][9])]

        def cols(items):
            return [it[0] for it in items], [it[1] for it in items], [it[2] for it in items], [it[3] for it in items]

        def on_device(items):
            cm, idx, ce, pf = cols(items)
            return dev(b"".join(cm)), torch.tensor(idx, dtype=torch.int64, device="cuda"), dev(b"".join(ce)), dev(b"".join(pf))

        n = len(items)
        assert K.verify_cell_kzg_proof_batch(*cols(items), ts) is True
        d_cm, d_idx, d_ce, d_pf = on_device(items)
        assert K.verify_cell_kzg_proof_batch_device(d_cm.data_ptr(), d_idx.data_ptr(), d_ce.data_ptr(), d_pf.data_ptr(), n, ts) is True
        v = K.CellVerifier(ts, n)
        try:
            res = v.enqueue(d_cm.data_ptr(), d_idx.data_ptr(), d_ce.data_ptr(), d_pf.data_ptr(), n)
            v.wait()
            assert (res.state, res.rc, res.ok) == (1, 0, 1)
            # one changed cell byte (the element stays below r: its low byte): false, and the per-item call names the item
            where = 130
            cm, k, cell, pf = items[where]
            changed = list(items)
            changed[where] = (cm, k, cell[:31] + bytes([cell[31] ^ 1]) + cell[32:], pf)
            assert K.verify_cell_kzg_proof_batch(*cols(changed), ts) is False
            c_cm, c_idx, c_ce, c_pf = on_device(changed)
            assert K.verify_cell_kzg_proof_batch_device(c_cm.data_ptr(), c_idx.data_ptr(), c_ce.data_ptr(), c_pf.data_ptr(), n, ts) is False
            res = v.enqueue(c_cm.data_ptr(), c_idx.data_ptr(), c_ce.data_ptr(), c_pf.data_ptr(), n)
            v.wait()
            assert (res.state, res.rc, res.ok) == (1, 0, 0)
        finally:
            v.free()
        each = K.verify_cell_kzg_proof_each(*cols(changed[124:]), ts)
        assert each == [(0, i != where - 124) for i in range(n - 124)]
        # an index of 128
        wrong = list(items[:3])
        wrong[1] = (wrong[1][0], 128, wrong[1][2], wrong[1][3])
        with pytest.raises(K.KzgError) as e:
            K.verify_cell_kzg_proof_batch(*cols(wrong), ts)
        assert e.value.rc == K.C_KZG_BADARGS
        # a cell element >= r
        nc = list(items[:3])
        nc[2] = (nc[2][0], nc[2][1], b"\xff" + nc[2][2][1:], nc[2][3])
        with pytest.raises(K.KzgError) as e:
            K.verify_cell_kzg_proof_batch(*cols(nc), ts)
        assert e.value.rc == K.C_KZG_BADARGS
        # r of the partials: the host transcript's, big-endian
        few = items[126:]
        part = K.cell_verify_partials(*cols(few), ts)
        r_host = K.cell_batch_challenge_host(*cols(few), ETH)
        assert part[:32] == r_host and int.from_bytes(r_host, "big") < R
        assert r_host == K.cell_batch_challenge_host(*cols(few), 0)
        # cells produced in c-kzg mode, presented unreversed in eth mode, do not verify
        le_items = [(cm, k, E.rev32(cell), pf) for cm, k, cell, pf in items[:4]]
        assert as_ckzg(ts, lambda: K.verify_cell_kzg_proof_batch(*cols(le_items), ts)) is True
        try:
            assert K.verify_cell_kzg_proof_batch(*cols(le_items), ts) is False
        except K.KzgError as e:                                   # (or an element that is not canonical read big-endian)
            assert e.rc == K.C_KZG_BADARGS
