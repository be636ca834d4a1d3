"""CPU: the parts of the cell verifier's grouped calls (lwkzg_cell_verifier_new_groups / _enqueue_groups) that need
no GPU. The new symbols in the header, the export list and the binding; the argument checks; the slice rule that the host's plan and
the device's slice table share, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/cell_groups_slice_rule_check.cpp); and the two host steps of a grouped enqueue through the host-only hook, on blocks put
together from tests/cell_verify_spec.py and the CPU oracle: an honest group answers what lwkzg_cell_verifier_host_steps answers on the
group alone, and a rejected group reads nothing behind what decides it."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cells_spec as S
from conftest import ROOT
from test_cell_verifier_cpu import MODES, NONE_BAD, _blocks, _hand_built_settings
from test_gpu_cell_verify import Poly

CSRC = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")
NEW_SYMBOLS = ["lwkzg_cell_verifier_new_groups", "lwkzg_cell_verifier_enqueue_groups", "lwkzg_cell_group_segmented_device",
               "lwkzg_cell_verifier_groups_host_steps"]
RULE_CASES = ["the rule", "boundary sizes with empty groups", "boundary sizes with repeated commitments", "sixty-five groups of one",
              "257 items in uneven groups", "1025 items in uneven groups", "a bad index first", "a bad index last"]


def test_new_symbols_are_declared_exported_and_bound(K):
    from lambdaworks_kzg_amd import capi
    header = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    l = K.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bC_KZG_RET %s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(l, name), name
    assert hasattr(K.CellVerifier, "enqueue_groups")
    # the grouped call's header comment no longer lists the form that does not block as out of scope
    assert "Out of scope: a non-blocking" not in header


def test_the_shared_slice_rule_against_the_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "cell_groups_slice_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "cell_groups_slice_rule_check.cpp")])
    run = subprocess.run([exe], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    assert out.strip().split("\n") == [c + " ok" for c in RULE_CASES], out


def test_argument_checks_need_no_gpu(K):
    l = K.lib()
    res = K.CellVerifyResult()
    ok, rc, off = (C.c_uint8 * 2)(7, 7), (C.c_int32 * 2)(-5, -5), (C.c_uint64 * 3)(0, 0, 0)
    assert l.lwkzg_cell_verifier_enqueue_groups(None, C.byref(res), ok, rc, None, None, None, None, None, 0, off, 2, None) == K.C_KZG_BADARGS
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, NONE_BAD)
    assert list(ok) == [7, 7] and list(rc) == [-5, -5]
    assert l.lwkzg_cell_verifier_enqueue_groups(None, None, ok, rc, None, None, None, None, None, 0, off, 2, None) == K.C_KZG_BADARGS
    s = K.KZGSettings()
    s.fs = s.g1_values = s.g2_values = None
    h = C.c_void_p(5)
    assert l.lwkzg_cell_verifier_new_groups(C.byref(h), C.byref(s), 64, 0) == K.C_KZG_BADARGS and not h.value
    h = C.c_void_p(5)
    assert l.lwkzg_cell_verifier_new_groups(C.byref(h), C.byref(s), 64, (1 << 30) + 1) == K.C_KZG_BADARGS and not h.value
    assert l.lwkzg_cell_verifier_new_groups(C.byref(h), None, 64, 4) == K.C_KZG_BADARGS
    assert l.lwkzg_cell_verifier_new_groups(None, C.byref(s), 64, 4) == K.C_KZG_BADARGS
    u32 = C.c_uint32
    one = (u32 * 2)()
    assert l.lwkzg_cell_group_segmented_device(None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, 4,
                                               off, 2, 1, 0xffffffff, None) == K.C_KZG_BADARGS
    # offsets that do not end at n, before anything touches a device
    assert l.lwkzg_cell_group_segmented_device(one, one, C.create_string_buffer(96), one, one, (u32 * 3)(), one, (u32 * 257)(), (u32 * 3)(),
                                               one, None, None, None, C.c_void_p(256), C.c_void_p(256), 2, off, 2, 1, 0xffffffff,
                                               None) == K.C_KZG_BADARGS
    assert l.lwkzg_cell_verifier_groups_host_steps(C.byref(res), ok, rc, None, off, 2, 2, (u32 * 3)(), (u32 * 2)(), None, None, None, None,
                                                   None, None, C.byref(s), S.MODE_REFERENCE) == K.C_KZG_BADARGS
    assert res.state == 1 and res.rc == K.C_KZG_BADARGS and list(ok) == [7, 7]


def _call(oracle, mode):
    """five groups: honest (5 items, 2 rows) | empty | a bad index | honest (3 items, 3 rows) | a faulty proof; the blocks as the device
    sends them down for an honest call, and each honest group's own blocks"""
    a, b, c = Poly.seeded(oracle, 3000), Poly.seeded(oracle, 3001), Poly.seeded(oracle, 3002)
    g0 = [a.item(5, mode), b.item(5, mode), a.item(64, mode), b.item(5, mode), a.item(127, mode)]
    g3 = [b.item(0, mode), a.item(5, mode), c.item(77, mode)]           # a and b again: rows of this group's own
    sizes = [len(g0), 0, 2, len(g3), 4]
    alone = {0: (g0,) + _blocks(oracle, g0, mode), 3: (g3,) + _blocks(oracle, g3, mode)}
    return sizes, alone


@pytest.mark.parametrize("mode", MODES)
def test_host_steps_an_honest_group_answers_as_the_batch_hook_on_the_group_alone(K, oracle, mode):
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle)
    sizes, alone = _call(oracle, mode)
    n, g = sum(sizes), len(sizes)
    off = [sum(sizes[:j]) for j in range(g + 1)]
    mode_code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    # rows: group 0 has two, group 3 three, group 4 (faulty) four; the dead and the empty group none
    row_base = [0, 2, 2, 2, 5, 9]
    m_total = row_base[-1]
    distinct = [bytes([0xc0]) + bytes(47)] * m_total
    first_item = [0] * m_total
    digests = bytearray(b"\x5a" * (32 * n))        # (what a rejected group would hash if it read them)
    sums, rli = bytearray(3 * 97 * g), bytearray(48 * g)
    for j, (items, dist, dig, first, sums97, rli48, _, _) in alone.items():
        rb = row_base[j]
        distinct[rb:rb + len(dist)] = dist
        first_item[rb:rb + len(dist)] = [off[j] + f for f in first]
        digests[32 * off[j]:32 * off[j + 1]] = dig
        sums[3 * 97 * j:3 * 97 * (j + 1)] = sums97
        rli[48 * j:48 * (j + 1)] = rli48
    first_item[5:9] = range(off[4], off[4] + 4)
    status = [0] * (2 * n)
    status[off[4] + 2] = mode_code                 # group 4: its third item's proof
    status[n + 3] = 0
    bad_words = [0, 0, 1, 0, 0]
    res, answers, partials = capi.cell_verifier_groups_host_steps(sizes, row_base, bad_words, status, first_item, bytes(digests),
                                                                  b"".join(distinct), bytes(sums), bytes(rli), C.byref(s), mode)
    assert (res.state, res.rc, res.ok, res.first_bad, res.m) == (1, K.C_KZG_OK, 0, 2, m_total)
    assert bytes(res.partials) == bytes(capi.CELL_VERIFY_PARTIAL_BYTES)
    assert answers == [(K.C_KZG_OK, True), (K.C_KZG_OK, True), (K.C_KZG_BADARGS, False), (K.C_KZG_OK, True), (mode_code, False)]
    for j in (1, 2, 4):
        assert partials[j] == bytes(capi.CELL_VERIFY_PARTIAL_BYTES), j
    for j, (items, dist, dig, first, sums97, rli48, _, _) in alone.items():
        want = capi.cell_verifier_host_steps(b"".join(dist), len(dist), dig, len(items), NONE_BAD, [0] * (2 * len(items)), first, sums97,
                                             rli48, C.byref(s), mode)
        assert (want.rc, want.ok) == (K.C_KZG_OK, 1)
        assert partials[j] == bytes(want.partials) and partials[j] != bytes(capi.CELL_VERIFY_PARTIAL_BYTES), j
    # a bad commitment counts for the group whose row it is: row 3 is group 3's second
    status[n + 3] = mode_code
    res, answers, partials = capi.cell_verifier_groups_host_steps(sizes, row_base, bad_words, status, first_item, bytes(digests),
                                                                  b"".join(distinct), bytes(sums), bytes(rli), C.byref(s), mode)
    assert answers == [(K.C_KZG_OK, True), (K.C_KZG_OK, True), (K.C_KZG_BADARGS, False), (mode_code, False), (mode_code, False)]
    assert partials[3] == bytes(capi.CELL_VERIFY_PARTIAL_BYTES) and partials[0] != partials[3]
    # one sum of group 0 corrupted (RLP in P's place): that group answers (OK, 0), its neighbours as before
    status[n + 3] = 0
    wrong = bytearray(sums)
    wrong[0:97] = sums[97:194]
    res, answers, _ = capi.cell_verifier_groups_host_steps(sizes, row_base, bad_words, status, first_item, bytes(digests), b"".join(distinct),
                                                           bytes(wrong), bytes(rli), C.byref(s), mode)
    assert answers[0] == (K.C_KZG_OK, False) and answers[3] == (K.C_KZG_OK, True) and res.first_bad == 0 and res.ok == 0
    del keep


@pytest.mark.parametrize("mode", MODES)
def test_host_steps_rejected_groups_read_nothing_behind_what_decides_them(K, oracle, mode):
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle)
    mode_code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    sizes = [0, 3, 0, 2, 0]
    n = 5
    # bad indices alone: neither the words nor first_item, neither digests nor commitments nor sums are given
    res, answers, partials = capi.cell_verifier_groups_host_steps(sizes, [0] * 6, [0, 1, 0, 1, 0], None, None, None, None, None, None, C.byref(s),
                                                                  mode)
    assert answers == [(K.C_KZG_OK, True), (K.C_KZG_BADARGS, False), (K.C_KZG_OK, True), (K.C_KZG_BADARGS, False), (K.C_KZG_OK, True)]
    assert (res.state, res.rc, res.ok, res.first_bad, res.m) == (1, K.C_KZG_OK, 0, 1, 0)
    assert partials == [bytes(capi.CELL_VERIFY_PARTIAL_BYTES)] * 5
    # a bad index is decided first, whatever the words say; a fault word needs the words and first_item, and nothing else
    row_base = [0, 0, 0, 0, 2, 2]
    status = [0] * (2 * n)
    status[1] = mode_code                          # an item of the dead group
    status[n + 1] = mode_code                      # group 3's second row
    res, answers, _ = capi.cell_verifier_groups_host_steps(sizes, row_base, [0, 1, 0, 0, 0], status, [3, 4], None, None, None, None,
                                                           C.byref(s), mode)
    assert answers == [(K.C_KZG_OK, True), (K.C_KZG_BADARGS, False), (K.C_KZG_OK, True), (mode_code, False), (K.C_KZG_OK, True)]
    assert (res.rc, res.ok, res.first_bad, res.m) == (K.C_KZG_OK, 0, 1, 2)
    # clean words make group 3 honest: its blocks are missing, and the hook says so
    with pytest.raises(K.KzgError) as e:
        capi.cell_verifier_groups_host_steps(sizes, row_base, [0, 1, 0, 0, 0], [0] * (2 * n), [3, 4], None, None, None, None, C.byref(s), mode)
    assert e.value.rc == K.C_KZG_BADARGS
    del keep


@pytest.mark.parametrize("mode", MODES)
def test_host_steps_one_fault_of_each_kind_in_the_order_the_synchronous_call_meets_them(K, oracle, mode):
    """The host steps are one piece of code (cells_verify_host.h) for the verifier and for lwkzg_verify_cell_kzg_proof_groups, so the
    synchronous call's decisions are reachable here: empty | a bad index | a cell element out of range at the group's last item | a
    bad commitment whose row is first seen at the group's second item | honest. The exact (rc, ok) vector, zero partials for the
    first four, and the hook's refusal of a call without ok_out and rc_out (partials alone are the synchronous
    lwkzg_cell_verify_groups_partials' form, never the hook's: refused with nothing written, as before the host steps were shared).
    Not reachable from here: the synchronous call hands the shared steps no first_item (first_fault then counts a bad commitment at
    item 0), and the hook refuses a NULL first_item; that one branch is covered by tests/test_gpu_cell_groups_one_host_side.py alone."""
    from lambdaworks_kzg_amd import capi
    s, keep = _hand_built_settings(capi, oracle)
    a, b = Poly.seeded(oracle, 3000), Poly.seeded(oracle, 3001)
    honest = [a.item(5, mode), b.item(5, mode), a.item(64, mode), b.item(5, mode), a.item(127, mode)]
    dist, dig, first, sums97, rli48, _, _ = _blocks(oracle, honest, mode)
    sizes = [0, 2, 3, 3, len(honest)]
    n, g = sum(sizes), len(sizes)
    off = [sum(sizes[:j]) for j in range(g + 1)]
    mode_code = K.C_KZG_BADARGS if mode == S.MODE_CKZG else K.C_KZG_ERROR
    row_base = [0, 0, 0, 2, 4, 4 + len(dist)]      # the empty and the dead group have no rows; groups 2 and 3 two each
    m_total = row_base[-1]
    distinct = [bytes([0xc0]) + bytes(47)] * 4 + list(dist)
    first_item = [off[2], off[2] + 1, off[3], off[3] + 1] + [off[4] + f for f in first]
    digests = b"\x5a" * (32 * off[4]) + dig        # (what a rejected group would hash if it read them)
    sums, rli = bytes(3 * 97 * 4) + sums97, bytes(48 * 4) + rli48
    status = [0] * (2 * n)
    status[off[3] - 1] = mode_code                 # group 2: an element of its last item's cell
    status[n + row_base[3] + 1] = mode_code        # group 3: its second row, first seen at its second item
    bad_words = [0, 1, 0, 0, 0]
    res, answers, partials = capi.cell_verifier_groups_host_steps(sizes, row_base, bad_words, status, first_item, digests, b"".join(distinct),
                                                                  sums, rli, C.byref(s), mode)
    assert answers == [(K.C_KZG_OK, True), (K.C_KZG_BADARGS, False), (mode_code, False), (mode_code, False), (K.C_KZG_OK, True)]
    assert (res.state, res.rc, res.ok, res.first_bad, res.m) == (1, K.C_KZG_OK, 0, 1, m_total)
    for j in range(4):
        assert partials[j] == bytes(capi.CELL_VERIFY_PARTIAL_BYTES), j
    alone = capi.cell_verifier_host_steps(b"".join(dist), len(dist), dig, len(honest), NONE_BAD, [0] * (2 * len(honest)), first, sums97, rli48,
                                          C.byref(s), mode)
    assert (alone.rc, alone.ok) == (K.C_KZG_OK, 1) and partials[4] == bytes(alone.partials) != bytes(capi.CELL_VERIFY_PARTIAL_BYTES)
    # ok_out = rc_out = NULL with partials_out given: BADARGS, the result complete, the partials untouched
    out = C.create_string_buffer(b"\x11" * (g * capi.CELL_VERIFY_PARTIAL_BYTES), g * capi.CELL_VERIFY_PARTIAL_BYTES)
    res = K.CellVerifyResult()
    u32 = C.c_uint32
    rc = K.lib().lwkzg_cell_verifier_groups_host_steps(C.byref(res), None, None, out, (C.c_uint64 * (g + 1))(*off), g, n,
                                                       (u32 * (g + 1))(*row_base), (u32 * g)(*bad_words), (C.c_int32 * (2 * n))(*status),
                                                       (u32 * m_total)(*first_item), digests, b"".join(distinct), sums, rli, C.byref(s), mode)
    assert rc == K.C_KZG_BADARGS and (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, NONE_BAD)
    assert out.raw == b"\x11" * (g * capi.CELL_VERIFY_PARTIAL_BYTES)
    del keep
