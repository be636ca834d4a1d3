"""CPU: what the blob calls of the cell verifier (lwkzg_cell_verifier_new_blobs / _enqueue_blobs / _enqueue_blobs_groups and the hook
lwkzg_blob_group_device) decide without a GPU: the four symbols in the header, the export list and the binding;
the argument checks that come before any device work; and the steps of the grouping kernel with the bodies of the expansion kernel,
run lane after lane by a stand-alone program under the sanitizers against plan_blobs."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW_SYMBOLS = ["lwkzg_cell_verifier_new_blobs", "lwkzg_cell_verifier_enqueue_blobs", "lwkzg_cell_verifier_enqueue_blobs_groups",
               "lwkzg_blob_group_device"]
GROUP_CASES = ["batch: one blob", "groups: one blob", "batch: 1 0 0 2 1 0 2", "groups: 1 0 0 2 1 0 2 in [0, 3, 0, 4, 0]",
               "groups: rows restart per group", "batch: 70 distinct commitments", "groups: 70 distinct commitments in one group",
               "groups: 512 blobs of 300 commitments in 5 groups", "batch: 512 blobs of 300 commitments"]


def test_the_four_symbols_are_declared_exported_and_wrapped(K):
    from lambdaworks_kzg_amd import capi
    header = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    exports = open(os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc", "exports.map")).read()
    assert re.search(r"\blwkzg_\*;", exports)
    dynamic = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    l = K.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bC_KZG_RET %s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(l, name), name
        assert re.search(r" T %s$" % name, dynamic, re.M), name
    for name in ("for_blobs", "enqueue_blobs", "enqueue_blobs_groups"):
        assert callable(getattr(K.CellVerifier, name)), name
    assert callable(capi.blob_group_device) and K.blob_group_device is capi.blob_group_device


def test_the_grouping_steps_equal_the_plan_under_the_sanitizers(tmp_path):
    """the steps k_blob_group runs between its barriers and the stores of k_blob_items_dev, lane after lane in three lane orders and
    with every key on one probe chain, on exactly sized blocks, against plan_blobs and blob_item_lists"""
    exe = str(tmp_path / "cell_blobs_group_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cell_blobs_group_check.cpp")])
    run = subprocess.run([exe], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    assert out.strip().split("\n") == [c + " ok" for c in GROUP_CASES], out


def test_new_blobs_checks_its_arguments_before_any_device_work(K):
    l = K.lib()
    s = K.KZGSettings()
    h = C.c_void_p(0x1234)
    assert l.lwkzg_cell_verifier_new_blobs(None, C.byref(s), 4, 1) == K.C_KZG_BADARGS
    assert l.lwkzg_cell_verifier_new_blobs(C.byref(h), None, 4, 1) == K.C_KZG_BADARGS and not h.value
    for max_blobs in (0, 513):
        h = C.c_void_p(0x1234)
        assert l.lwkzg_cell_verifier_new_blobs(C.byref(h), C.byref(s), max_blobs, 1) == K.C_KZG_BADARGS and not h.value, max_blobs
        assert b"1 .. 512" in l.lwkzg_last_error()
    h = C.c_void_p(0x1234)
    assert l.lwkzg_cell_verifier_new_blobs(C.byref(h), C.byref(s), 4, (1 << 30) + 1) == K.C_KZG_BADARGS and not h.value


def test_the_enqueue_calls_refuse_a_null_handle_and_a_null_result(K):
    l = K.lib()
    ok, rc = (C.c_uint8 * 2)(7, 7), (C.c_int32 * 2)(-5, -5)
    off = (C.c_uint64 * 3)(0, 1, 2)
    res = K.CellVerifyResult()
    res.state = 9
    assert l.lwkzg_cell_verifier_enqueue_blobs(None, C.byref(res), None, None, None, 0, None) == K.C_KZG_BADARGS
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, 0xffffffff)
    res.state = 9
    assert l.lwkzg_cell_verifier_enqueue_blobs_groups(None, C.byref(res), ok, rc, None, None, None, None, 0, off, 2, None) == K.C_KZG_BADARGS
    assert (res.state, res.rc, res.ok, res.first_bad) == (1, K.C_KZG_BADARGS, 0, 0xffffffff)
    assert list(ok) == [7, 7] and list(rc) == [-5, -5]
    fake = C.create_string_buffer(256)     # no verifier's magic either
    assert l.lwkzg_cell_verifier_enqueue_blobs(fake, None, None, None, None, 0, None) == K.C_KZG_BADARGS
    assert l.lwkzg_cell_verifier_enqueue_blobs_groups(fake, None, ok, rc, None, None, None, None, 0, off, 2, None) == K.C_KZG_BADARGS
    assert l.lwkzg_cell_verifier_enqueue_blobs(fake, C.byref(res), None, None, None, 0, None) == K.C_KZG_BADARGS and res.state == 1
