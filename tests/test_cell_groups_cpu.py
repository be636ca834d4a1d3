"""CPU: the grouped EIP-7594 cell proof verification (lwkzg_verify_cell_kzg_proof_groups, _device, lwkzg_cell_verify_groups_partials) as
far as it goes without a GPU: the host's plan, lambdaworks_kzg_amd/csrc/cell_groups_plan.h, as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/cell_groups_plan_check.cpp: the offsets' checks, empty groups at the front, in the
middle and at the end, a commitment repeated inside a group and across two groups, the slice tables of group sizes 0, 1, 64, 65, 128,
129, the dead flag), and every call-level C_KZG_BADARGS on a hand-built settings object, with nothing written to the outputs."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")
CASES = ["offsets", "empty groups and rows that restart", "repeats inside a group", "slice tables", "dead flag"]


def test_the_plan_of_a_call_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "cell_groups_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "cell_groups_plan_check.cpp")])
    run = subprocess.run([exe], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    assert out.strip().split("\n") == [c + " ok" for c in CASES], out


def test_call_level_argument_checks_need_no_gpu_and_write_nothing(K):
    l = K.lib()
    s = K.KZGSettings()           # hand-made: no context behind it
    pb = K.capi.CELL_VERIFY_PARTIAL_BYTES
    ok = (C.c_uint8 * 3)(7, 7, 7)
    rc = (C.c_int32 * 3)(-5, -5, -5)
    part = C.create_string_buffer(b"\x55" * (3 * pb), 3 * pb)
    idx = (C.c_uint64 * 2)(0, 1)
    comm, cells, proofs = bytes(96), bytes(4096), bytes(96)
    dev = C.c_void_p(4096)        # never dereferenced: every call below is refused, or has nothing to do, before it is looked at
    u64 = C.c_uint64

    def untouched():
        return list(ok) == [7, 7, 7] and list(rc) == [-5, -5, -5] and part.raw == b"\x55" * (3 * pb)

    def calls(off, g, n=2, s_ref=C.byref(s), outs=(ok, rc, part), items=(comm, idx, cells, proofs)):
        d = tuple(None if a is None else dev for a in items)
        return [l.lwkzg_verify_cell_kzg_proof_groups(outs[0], outs[1], *items, n, off, g, s_ref),
                l.lwkzg_verify_cell_kzg_proof_groups_device(outs[0], outs[1], *d, n, off, g, s_ref, None),
                l.lwkzg_cell_verify_groups_partials(outs[2], *items, n, off, g, s_ref)]

    good = (u64 * 3)(0, 1, 2)
    bad3 = [K.C_KZG_BADARGS] * 3
    # s NULL, whatever else
    assert calls(good, 2, s_ref=None) == bad3
    assert calls(None, 0, n=0, s_ref=None) == bad3
    # the outputs or the offsets NULL with g > 0
    assert calls(None, 2) == bad3
    assert calls(good, 2, outs=(None, rc, None)) == bad3
    assert calls(good, 2, outs=(ok, None, None))[:2] == bad3[:2]
    # an item array NULL with n > 0
    for hole in range(4):
        items = [comm, idx, cells, proofs]
        items[hole] = None
        assert calls(good, 2, items=tuple(items)) == bad3, hole
    # offsets that do not start at 0, do not end at n, or do not ascend; g == 0 with n > 0
    assert calls((u64 * 3)(1, 1, 2), 2) == bad3
    assert calls((u64 * 3)(0, 1, 3), 2) == bad3
    assert calls((u64 * 3)(0, 1, 1), 2) == bad3
    assert calls((u64 * 4)(0, 2, 1, 2), 3) == bad3
    assert calls((u64 * 4)(0, 1 << 63, 1, 2), 3) == bad3
    assert calls(good, 0) == bad3
    assert calls(None, 0) == bad3
    assert untouched()
    # g == 0 with n == 0: C_KZG_OK, nothing written -- with arguments and without
    assert calls((u64 * 1)(0), 0, n=0) == [K.C_KZG_OK] * 3
    assert calls(None, 0, n=0, outs=(None, None, None), items=(None, None, None, None)) == [K.C_KZG_OK] * 3
    assert untouched()
    # what the batch call refuses as a whole is refused the same way: settings without a context
    batch_ok = C.c_bool(True)
    want = l.lwkzg_verify_cell_kzg_proof_batch(C.byref(batch_ok), comm, idx, cells, proofs, 2, C.byref(s))
    assert want == K.C_KZG_ERROR
    assert l.lwkzg_verify_cell_kzg_proof_groups(ok, rc, comm, idx, cells, proofs, 2, good, 2, C.byref(s)) == want
    assert l.lwkzg_cell_verify_groups_partials(part, comm, idx, cells, proofs, 2, good, 2, C.byref(s)) == want
    # empty groups alone are the batch call's n == 0: answered without a context
    assert l.lwkzg_verify_cell_kzg_proof_groups(ok, rc, None, None, None, None, 0, (u64 * 4)(0, 0, 0, 0), 3, C.byref(s)) == K.C_KZG_OK
    assert list(ok) == [1, 1, 1] and list(rc) == [K.C_KZG_OK] * 3


def test_python_wrappers_are_exported(K):
    for name in ("verify_cell_kzg_proof_groups", "verify_cell_kzg_proof_groups_device", "cell_verify_groups_partials"):
        assert callable(getattr(K, name)) and getattr(K.capi, name) is getattr(K, name)
    hdr = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    for name in ("lwkzg_verify_cell_kzg_proof_groups(", "lwkzg_verify_cell_kzg_proof_groups_device(", "lwkzg_cell_verify_groups_partials("):
        assert name in hdr
