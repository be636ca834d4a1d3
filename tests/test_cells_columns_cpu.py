"""CPU: what the column calls (lwkzg_compute_cells_and_kzg_proofs_columns / lwkzg_recover_cells_and_kzg_proofs_columns and their device
forms) decide without a GPU: the four symbols in the header, the export list and the binding; the plan
(cells_columns_plan.h) under the sanitizers; every argument error, which leaves a filled output buffer alone; the empty calls."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW_SYMBOLS = ["lwkzg_compute_cells_and_kzg_proofs_columns", "lwkzg_compute_cells_and_kzg_proofs_columns_device",
               "lwkzg_recover_cells_and_kzg_proofs_columns", "lwkzg_recover_cells_and_kzg_proofs_columns_device"]
WRAPPERS = [name[len("lwkzg_"):] for name in NEW_SYMBOLS]
BLOB, CELL = bytes(4096 * 32), bytes(2048)
UNTOUCHED = 0x5a


def _filled(size):
    return C.create_string_buffer(bytes([UNTOUCHED]) * size, size)


def _u64(values):
    return (C.c_uint64 * max(len(values), 1))(*values)


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
    for name in WRAPPERS:
        assert callable(getattr(capi, name)) and getattr(K, name) is getattr(capi, name), name
    section = header[header.index("Chosen columns only"):header.index("lwkzg_compute_cells_and_kzg_proofs_columns(")]
    assert "strictly ascending" in " ".join(section.replace("*", " ").split())


PLAN_CASES = ["chunk: the three capacities hold and m + 1 breaks one",
              "c = 128: 8 / 512 / 512 blobs per chunk and 128 m or 2 m slots, as the full calls have them",
              "reserve: every slot a pass touches, and no more than a launch set",
              "engine: FK20 iff it is on, proofs are wanted and n c >= 128 min_blobs; monotone in n and in c",
              "host slice: whole chunks or the whole call, at least 64 blobs when the call has them, within the staging bound"]


def test_the_plan_holds_its_capacities_and_the_full_calls_figures_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "cells_columns_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cells_columns_plan_check.cpp")])
    run = subprocess.run([exe], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    assert out.strip().split("\n") == [c + " ok" for c in PLAN_CASES], out


BAD_LISTS = [("no list", None, 2), ("no columns", [0], 0), ("129 columns", list(range(128)) + [128], 129), ("an index of 128", [5, 128], 2),
             ("an index of 2^63", [5, 2 ** 63], 2), ("descending", [7, 3], 2), ("a column twice", [3, 3], 2),
             ("ascending but for the last", list(range(0, 100, 2)) + [97], 51)]


def _compute(l, s, form, cells, proofs, blobs, n, cols, num, with_bad=True):
    cols = None if cols is None else _u64(cols)
    sref = None if s is None else C.byref(s)
    if form == "host":
        return l.lwkzg_compute_cells_and_kzg_proofs_columns(cells, proofs, blobs, n, cols, num, sref, None)
    return l.lwkzg_compute_cells_and_kzg_proofs_columns_device(cells, proofs, blobs, n, cols, num, sref, None, None)


def test_compute_argument_errors_and_the_empty_call_need_no_gpu(K):
    l = K.lib()
    s = K.KZGSettings()
    size = 2 * 2 * 2048
    for form in ["host", "device"]:
        cells, proofs = _filled(size), _filled(2 * 2 * 48)
        # (the device form's pointers are never followed: every check comes first)
        cp, pp, bp = (cells, proofs, BLOB * 2) if form == "host" else (C.addressof(cells), C.addressof(proofs), 16)
        for what, cols, num in BAD_LISTS:
            assert _compute(l, s, form, cp, pp, bp, 2, cols, num) == K.C_KZG_BADARGS, (form, what)
        assert _compute(l, s, form, cp, pp, None, 2, [0, 1], 2) == K.C_KZG_BADARGS      # no blobs
        assert _compute(l, s, form, None, None, bp, 2, [0, 1], 2) == K.C_KZG_BADARGS    # neither output
        assert _compute(l, None, form, cp, pp, bp, 2, [0, 1], 2) == K.C_KZG_BADARGS     # no settings
        # n == 0: fine, whatever the other pointers are
        assert _compute(l, s, form, cp, pp, None, 0, None, 0) == K.C_KZG_OK
        assert _compute(l, s, form, None, None, None, 0, [9, 3], 200) == K.C_KZG_OK
        assert cells.raw == bytes([UNTOUCHED]) * size and proofs.raw == bytes([UNTOUCHED]) * (2 * 2 * 48), form


def _recover(l, s, form, cells_out, proofs, idx, cells, num_cells, n, cols, num):
    cols = None if cols is None else _u64(cols)
    idx = None if idx is None else _u64(idx)
    sref = None if s is None else C.byref(s)
    if form == "host":
        return l.lwkzg_recover_cells_and_kzg_proofs_columns(cells_out, proofs, idx, cells, num_cells, n, cols, num, sref, None)
    return l.lwkzg_recover_cells_and_kzg_proofs_columns_device(cells_out, proofs, idx, cells, num_cells, n, cols, num, sref, None, None)


def test_recover_argument_errors_and_the_empty_call_need_no_gpu(K):
    l = K.lib()
    s = K.KZGSettings()
    given = list(range(0, 128, 2))
    size = 2 * 2 * 2048
    for form in ["host", "device"]:
        out, proofs = _filled(size), _filled(2 * 2 * 48)
        op, pp, cp = (out, proofs, CELL * (2 * 64)) if form == "host" else (C.addressof(out), C.addressof(proofs), 16)
        for what, cols, num in BAD_LISTS:
            assert _recover(l, s, form, op, pp, given, cp, 64, 2, cols, num) == K.C_KZG_BADARGS, (form, what)
        # every argument error of the full call
        assert _recover(l, s, form, op, pp, None, cp, 64, 2, [1, 3], 2) == K.C_KZG_BADARGS
        assert _recover(l, s, form, op, pp, given, None, 64, 2, [1, 3], 2) == K.C_KZG_BADARGS
        assert _recover(l, s, form, None, None, given, cp, 64, 2, [1, 3], 2) == K.C_KZG_BADARGS
        assert _recover(l, s, form, op, pp, given[:63], cp, 63, 2, [1, 3], 2) == K.C_KZG_BADARGS          # too few given
        assert _recover(l, s, form, op, pp, given[:63] + [128], cp, 64, 2, [1, 3], 2) == K.C_KZG_BADARGS  # a given index of 128
        assert _recover(l, s, form, op, pp, [2, 0] + given[2:], cp, 64, 2, [1, 3], 2) == K.C_KZG_BADARGS  # given not ascending
        assert _recover(l, None, form, op, pp, given, cp, 64, 2, [1, 3], 2) == K.C_KZG_BADARGS
        # n == 0
        assert _recover(l, s, form, op, pp, None, None, 0, 0, None, 0) == K.C_KZG_OK
        assert _recover(l, s, form, None, None, given, None, 3, 0, [4, 4], 300) == K.C_KZG_OK
        assert out.raw == bytes([UNTOUCHED]) * size and proofs.raw == bytes([UNTOUCHED]) * (2 * 2 * 48), form


def test_the_python_wrappers_return_one_entry_per_column(K):
    from lambdaworks_kzg_amd import capi
    cells = b"".join(bytes([i]) * 2048 for i in range(6))
    proofs = b"".join(bytes([i]) * 48 for i in range(6))
    got = capi._columns_split(cells, proofs, 2, 3)
    assert [[c[0] for c in cs] for cs, _ in got] == [[0, 1, 2], [3, 4, 5]] and all(len(c) == 2048 for cs, _ in got for c in cs)
    assert [[p[0] for p in ps] for _, ps in got] == [[0, 1, 2], [3, 4, 5]] and all(len(p) == 48 for _, ps in got for p in ps)
    assert capi._columns_split(None, proofs, 2, 3)[1][0] is None
