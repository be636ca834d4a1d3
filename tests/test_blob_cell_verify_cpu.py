"""CPU: what the cell proof verification of whole blobs (lwkzg_verify_blob_cell_kzg_proofs_batch / _groups and their forms; DESIGN.md
section 4s) decides without a GPU: the six symbols in the header, the export list and the binding; every argument error of both
calls; the empty calls; the offset rules, which count blobs."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW_SYMBOLS = ["lwkzg_verify_blob_cell_kzg_proofs_batch", "lwkzg_verify_blob_cell_kzg_proofs_batch_device", "lwkzg_blob_cell_verify_partials",
               "lwkzg_verify_blob_cell_kzg_proofs_groups", "lwkzg_verify_blob_cell_kzg_proofs_groups_device",
               "lwkzg_blob_cell_verify_groups_partials"]
WRAPPERS = ["verify_blob_cell_kzg_proofs_batch", "verify_blob_cell_kzg_proofs_batch_device", "verify_blob_cell_kzg_proofs_groups",
            "verify_blob_cell_kzg_proofs_groups_device", "blob_cell_verify_partials", "blob_cell_verify_groups_partials"]
BLOB, CM, PROOFS = bytes(4096 * 32), bytes(48), bytes(128 * 48)
UNTOUCHED = 0x5a


def _filled(size):
    return C.create_string_buffer(bytes([UNTOUCHED]) * size, size)


def test_the_six_symbols_are_declared_exported_and_wrapped(K):
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
    for name in WRAPPERS:
        assert callable(getattr(capi, name)) and getattr(K, name) is getattr(capi, name), name
    assert "256 KiB" in header[header.index("Cell proofs of WHOLE BLOBS"):header.index("lwkzg_verify_blob_cell_kzg_proofs_batch(")]


PLAN_CASES = ["batch: one blob", "batch: the same blob twice", "batch: A B A", "batch: B A A C B A C", "batch: 65 blobs of three commitments",
              "groups: one blob", "groups: [0, 1, 1, 3, 6]", "groups: empty groups at the front, in the middle and at the end",
              "groups: rows restart per group", "groups: everything in one group", "groups: one group per blob", "groups: 70 rows in a group"]


def test_the_closed_form_lists_equal_the_plan_of_the_expanded_items_under_the_sanitizers(tmp_path):
    """what k_blob_items writes from the per-blob tables, store by store on exactly sized blocks, against group_items and plan_groups"""
    exe = str(tmp_path / "cell_blobs_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cell_blobs_plan_check.cpp")])
    run = subprocess.run([exe], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    assert out.strip().split("\n") == [c + " ok" for c in PLAN_CASES], out


def test_batch_argument_errors_and_the_empty_call_need_no_gpu(K):
    from lambdaworks_kzg_amd import capi
    l = K.lib()
    s = K.KZGSettings()
    ok = C.c_bool(False)
    # n == 0: true, whatever the arrays
    assert l.lwkzg_verify_blob_cell_kzg_proofs_batch(C.byref(ok), None, None, None, 0, C.byref(s)) == K.C_KZG_OK and ok.value is True
    ok.value = False
    assert l.lwkzg_verify_blob_cell_kzg_proofs_batch_device(C.byref(ok), None, None, None, 0, C.byref(s), None) == K.C_KZG_OK
    assert ok.value is True
    out = _filled(capi.CELL_VERIFY_PARTIAL_BYTES)
    assert l.lwkzg_blob_cell_verify_partials(out, None, None, None, 0, C.byref(s)) == K.C_KZG_OK
    assert out.raw == bytes([UNTOUCHED]) * capi.CELL_VERIFY_PARTIAL_BYTES
    # an array NULL with n > 0
    for args in [(None, CM, PROOFS), (BLOB, None, PROOFS), (BLOB, CM, None)]:
        ok.value = True
        assert l.lwkzg_verify_blob_cell_kzg_proofs_batch(C.byref(ok), *args, 1, C.byref(s)) == K.C_KZG_BADARGS, args
        assert ok.value is False
        assert l.lwkzg_blob_cell_verify_partials(out, *args, 1, C.byref(s)) == K.C_KZG_BADARGS
    for args in [(None, 16, 16), (16, None, 16), (16, 16, None)]:   # (never read: the check comes first)
        ok.value = True
        assert l.lwkzg_verify_blob_cell_kzg_proofs_batch_device(C.byref(ok), *args, 1, C.byref(s), None) == K.C_KZG_BADARGS, args
        assert ok.value is False
    # ok or s NULL
    assert l.lwkzg_verify_blob_cell_kzg_proofs_batch(None, BLOB, CM, PROOFS, 1, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_verify_blob_cell_kzg_proofs_batch_device(None, 16, 16, 16, 1, C.byref(s), None) == K.C_KZG_BADARGS
    ok.value = True
    assert l.lwkzg_verify_blob_cell_kzg_proofs_batch(C.byref(ok), BLOB, CM, PROOFS, 1, None) == K.C_KZG_BADARGS and ok.value is False
    ok.value = True
    assert l.lwkzg_verify_blob_cell_kzg_proofs_batch_device(C.byref(ok), 16, 16, 16, 1, None, None) == K.C_KZG_BADARGS and ok.value is False
    assert l.lwkzg_blob_cell_verify_partials(None, BLOB, CM, PROOFS, 1, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_blob_cell_verify_partials(out, BLOB, CM, PROOFS, 1, None) == K.C_KZG_BADARGS
    assert out.raw == bytes([UNTOUCHED]) * capi.CELL_VERIFY_PARTIAL_BYTES
    # more blobs than the pipelines count items for
    ok.value = True
    assert l.lwkzg_verify_blob_cell_kzg_proofs_batch(C.byref(ok), BLOB, CM, PROOFS, 2 ** 24, C.byref(s)) == K.C_KZG_BADARGS
    assert ok.value is False


def _groups(l, s, blobs, cm, pf, n, offsets, g, ok=True, rc=True, form="host"):
    """(return code, ok_out, rc_out) with both outputs pre-filled, so that a write shows"""
    okb, rcb = (C.c_uint8 * 8)(*[UNTOUCHED] * 8), (C.c_int32 * 8)(*[UNTOUCHED] * 8)
    off = None if offsets is None else (C.c_uint64 * len(offsets))(*offsets)
    args = (okb if ok else None, rcb if rc else None, blobs, cm, pf, n, off, g, C.byref(s) if s is not None else None)
    got = l.lwkzg_verify_blob_cell_kzg_proofs_groups(*args) if form == "host" else l.lwkzg_verify_blob_cell_kzg_proofs_groups_device(*args, None)
    return got, list(okb), list(rcb)


def test_groups_argument_errors_offset_rules_and_the_empty_calls_need_no_gpu(K):
    from lambdaworks_kzg_amd import capi
    l = K.lib()
    s = K.KZGSettings()
    nothing = [UNTOUCHED] * 8
    part = capi.CELL_VERIFY_PARTIAL_BYTES
    for form, (b, c, p) in [("host", (BLOB * 3, CM * 3, PROOFS * 3)), ("device", (16, 16, 16))]:
        # g == 0 with n == 0: fine, nothing written; g == 0 with n > 0: the offsets cannot cover the blobs
        assert _groups(l, s, None, None, None, 0, None, 0, form=form) == (K.C_KZG_OK, nothing, nothing)
        assert _groups(l, s, b, c, p, 3, [0], 0, form=form) == (K.C_KZG_BADARGS, nothing, nothing)
        # empty groups alone answer (C_KZG_OK, 1) each
        got, ok, rc = _groups(l, s, None, None, None, 0, [0, 0, 0, 0], 3, form=form)
        assert got == K.C_KZG_OK and ok[:4] == [1, 1, 1, UNTOUCHED] and rc[:4] == [K.C_KZG_OK] * 3 + [UNTOUCHED]
        # NULL arguments
        assert _groups(l, None, b, c, p, 3, [0, 3], 1, form=form) == (K.C_KZG_BADARGS, nothing, nothing)
        assert _groups(l, s, b, c, p, 3, [0, 3], 1, ok=False, form=form)[0] == K.C_KZG_BADARGS
        assert _groups(l, s, b, c, p, 3, [0, 3], 1, rc=False, form=form)[0] == K.C_KZG_BADARGS
        assert _groups(l, s, b, c, p, 3, None, 1, form=form) == (K.C_KZG_BADARGS, nothing, nothing)
        for args in [(None, c, p), (b, None, p), (b, c, None)]:
            assert _groups(l, s, *args, 3, [0, 3], 1, form=form) == (K.C_KZG_BADARGS, nothing, nothing), args
        # the offsets count BLOBS: g + 1 ascending values from 0 to n
        for offsets in [[1, 3], [0, 2], [0, 4], [0, 2, 1, 3], [0, 384], [0, 2 ** 63, 3], [3, 0]]:
            g = len(offsets) - 1
            assert _groups(l, s, b, c, p, 3, offsets, g, form=form) == (K.C_KZG_BADARGS, nothing, nothing), offsets
        assert _groups(l, s, b, c, p, 2 ** 24, [0, 2 ** 24], 1, form=form) == (K.C_KZG_BADARGS, nothing, nothing)
    # the partials hook: the same list, and out NULL with g > 0
    out = _filled(3 * part)
    off = (C.c_uint64 * 4)(0, 0, 0, 0)
    assert l.lwkzg_blob_cell_verify_groups_partials(out, None, None, None, 0, off, 3, C.byref(s)) == K.C_KZG_OK
    assert out.raw == bytes(3 * part)           # empty groups: zero bytes, as the hook over items writes them
    assert l.lwkzg_blob_cell_verify_groups_partials(None, None, None, None, 0, off, 3, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_blob_cell_verify_groups_partials(None, None, None, None, 0, None, 0, C.byref(s)) == K.C_KZG_OK
    out = _filled(part)
    bad = (C.c_uint64 * 2)(0, 2)
    assert l.lwkzg_blob_cell_verify_groups_partials(out, BLOB * 3, CM * 3, PROOFS * 3, 3, bad, 1, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_blob_cell_verify_groups_partials(out, None, CM * 3, PROOFS * 3, 3, (C.c_uint64 * 2)(0, 3), 1, C.byref(s)) == K.C_KZG_BADARGS
    assert l.lwkzg_blob_cell_verify_groups_partials(out, BLOB * 3, CM * 3, PROOFS * 3, 3, (C.c_uint64 * 2)(0, 3), 1, None) == K.C_KZG_BADARGS
    assert out.raw == bytes([UNTOUCHED]) * part


def test_the_python_wrappers_check_their_shapes(K):
    import pytest
    with pytest.raises(ValueError):
        K.verify_blob_cell_kzg_proofs_batch(BLOB, CM, PROOFS[:-48], None)
    with pytest.raises(ValueError):
        K.verify_blob_cell_kzg_proofs_groups(BLOB * 2, CM * 2, PROOFS * 2, [1], None)
    with pytest.raises(ValueError):
        K.blob_cell_verify_groups_partials(BLOB * 2, CM * 2, PROOFS * 2, [1, 2], None)
