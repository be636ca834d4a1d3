"""GPU: the grouped cell proof calls have ONE host side (cells_verify_host.h; DESIGN.md sections 4q, 4r). The synchronous
lwkzg_verify_cell_kzg_proof_groups, its _device form and lwkzg_cell_verify_groups_partials are held against the cell verifier's
enqueue_groups on the same five-group call, byte for byte, and each against lwkzg_verify_cell_kzg_proof_batch on each range alone.
Group sizes 0, 1, 2, 65 and 3: the group of 65 has its fault at item 64, in the second slice of its sums. Every fault kind appears once
over the two calls of a mode; the bad commitment is shared by bytes between two groups and condemns both, each at its own row."""
import pytest

import blobs as B
import cells_spec as S
from conftest import R
from test_gpu_cell_verify import MODES, _mode, _x_off_the_curve
from test_gpu_cell_verify_async import _Dev

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 65, 3]
ZERO = bytes(32 + 4 * 97)
ORDER3 = bytes([0x80]) + bytes(47)            # (0, 2): on the curve, of order 3


@pytest.fixture(scope="module")
def library_cells(K, gpu_setup):
    """the 128 cells of two blobs with their proofs, made by the library: 256 items per mode"""
    out = {}
    for mode in MODES:
        blobs = b"".join(B.synthetic_blob(970 + i, big_endian=mode == S.MODE_REFERENCE) for i in range(2))
        with _mode(K, gpu_setup, mode):
            comms = K.blob_to_kzg_commitment_batch(blobs, gpu_setup)
            made = K.compute_cells_and_kzg_proofs_batch(blobs, gpu_setup)
        out[mode] = [(comms[b], k, made[b][0][k], made[b][1][k]) for b in range(2) for k in range(128)]
    return out


@pytest.fixture(scope="module")
def verifier(K, gpu_setup):
    v = K.CellVerifier(gpu_setup, 128, 8)
    yield v
    v.free()


def _call(items, mode, faults):
    """the five groups, alternating between the two blobs so that every group has its own rows; returns the groups and, per group, the
    (rc, ok) it must answer (code: the mode's rejection code)"""
    mixed = [items[(i % 2) * 128 + i // 2] for i in range(96)]
    groups, at = [], 0
    for m in SIZES:
        groups.append(list(mixed[at:at + m]))
        at += m
    c, k, cell, proof = groups[3][64]
    if faults == "commitments":
        groups[1][0] = (groups[1][0][0], 128) + groups[1][0][2:]                          # a bad index
        groups[2][1] = (ORDER3,) + groups[2][1][1:]                                       # a bad commitment: row 1 of group 2 ...
        groups[3][64] = (ORDER3, k, cell, proof)                                          # ... and row 2 of group 3, by the same bytes
        want = ["ok", "index", "code", "code", "ok"]
    else:
        groups[1][0] = groups[1][0][:3] + (_x_off_the_curve(),)                           # a proof off the curve
        groups[3][64] = (c, k, cell[:64] + S.to_bytes(R, mode) + cell[96:], proof)        # a cell element not below r
        groups[4][1] = groups[4][1][:2] + (groups[4][2][2], groups[4][1][3])              # a tampered cell: summed, and false
        want = ["ok", "code", "ok", "code", "false"]
    return groups, want


@pytest.mark.parametrize("faults", ["commitments", "items"])
@pytest.mark.parametrize("mode", MODES)
def test_synchronous_and_verifier_answers_are_the_same_bytes(K, gpu_setup, verifier, library_cells, mode, faults):
    groups, want = _call(library_cells[mode], mode, faults)
    code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    want = [{"ok": (K.C_KZG_OK, True), "false": (K.C_KZG_OK, False), "index": (K.C_KZG_BADARGS, False), "code": (code, False)}[w] for w in want]
    d = _Dev([it for grp in groups for it in grp])
    with _mode(K, gpu_setup, mode):
        ans = verifier.enqueue_groups(*d.ptrs(), d.n, SIZES)
        verifier.wait()
        host = K.verify_cell_kzg_proof_groups(groups, gpu_setup)
        device = K.verify_cell_kzg_proof_groups_device(*d.ptrs(), d.n, SIZES, gpu_setup)
        partials = K.cell_verify_groups_partials(groups, gpu_setup)
        alone, alone_partials = [], []
        for grp in groups:
            cols = [[it[q] for it in grp] for q in range(4)]
            try:
                alone.append((K.C_KZG_OK, K.verify_cell_kzg_proof_batch(*cols, gpu_setup)))
            except K.KzgError as e:
                alone.append((e.rc, False))
            try:
                alone_partials.append(K.cell_verify_partials(*cols, gpu_setup) if grp else ZERO)
            except K.KzgError:
                alone_partials.append(ZERO)
    print(mode, faults, "verifier", ans.answers(), "host", host, "device", device, "alone", alone)
    assert ans.result.state == 1 and verifier.pending() == 0
    assert host == device == ans.answers() == alone == want
    assert partials == ans.partials() == alone_partials
    assert [p == ZERO for p in partials] == [a[0] != K.C_KZG_OK or not grp for a, grp in zip(want, groups)]
    bad = [j for j, a in enumerate(want) if a != (K.C_KZG_OK, True)]
    assert (ans.result.rc, ans.result.ok, ans.result.first_bad) == (K.C_KZG_OK, 0, bad[0])
    assert bytes(ans.result.partials) == ZERO
