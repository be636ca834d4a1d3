"""CPU: the mixed recovery (lwkzg_recover_cells_and_kzg_proofs_mixed, _mixed_device: every blob its own index set). The host side of
the sets, lambdaworks_kzg_amd/csrc/recover_sets.h, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/recover_sets_check.cpp: de-duplication in order of first occurrence, cell offsets, every argument error naming its blob,
n = 0, the one set of a shared-set call), and the argument checks of both entry points on a hand-built settings object, which need no GPU."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")

CASES = [
    "deduplication [A, B, A]", "deduplication [B, A, B, A]", "offsets 64, 128, 65",
    "count 63", "count 63 in front", "count 129", "count 129 in front", "index 128", "index 128 in front",
    "index 2^64 - 1", "index 2^64 - 1 in front", "a repeated index", "a repeated index in front",
    "a descending pair", "a descending pair in front", "n = 0", "one list", "shared set, n = 3",
]


def test_the_sets_of_a_call_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "recover_sets_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "recover_sets_check.cpp")])
    run = subprocess.run([exe], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    assert out.strip().split("\n") == [c + " ok" for c in CASES], out


def test_argument_checks_need_no_gpu(K):
    l = K.lib()
    s = K.KZGSettings()
    ps = C.byref(s)
    n = 3
    cells_out, proofs = C.create_string_buffer(n * 128 * 2048), C.create_string_buffer(n * 128 * 48)
    untouched = 12345

    def both(lists, out=(cells_out, proofs), cells=True, counts=True, indices=True, settings=ps, n_blobs=None):
        """[(rc, first_bad)] of the host form and [(rc, None)] of the device form on the lists of one call"""
        flat = [k for lst in lists for k in lst]
        idx = (C.c_uint64 * max(len(flat), 1))(*flat) if indices else None
        num = (C.c_size_t * max(len(lists), 1))(*[len(lst) for lst in lists]) if counts else None
        ce = bytes(max(len(flat), 1) * 2048) if cells else None
        nb = len(lists) if n_blobs is None else n_blobs
        first_bad = C.c_size_t(untouched)
        host = l.lwkzg_recover_cells_and_kzg_proofs_mixed(out[0], out[1], idx, ce, num, nb, settings, C.byref(first_bad))
        dev = l.lwkzg_recover_cells_and_kzg_proofs_mixed_device(C.cast(out[0], C.c_void_p), C.cast(out[1], C.c_void_p), idx,
                                                                C.cast(C.c_char_p(ce), C.c_void_p) if cells else None, num, nb, settings,
                                                                None, None)
        # without first_bad the host form answers the same
        assert l.lwkzg_recover_cells_and_kzg_proofs_mixed(out[0], out[1], idx, ce, num, nb, settings, None) == host
        return [(host, first_bad.value), (dev, None)]

    def refused(at):
        return [(K.C_KZG_BADARGS, at), (K.C_KZG_BADARGS, None)]

    a, b = list(range(64)), list(range(28, 128))
    # n == 0 answers OK without touching anything, whatever else is passed; s NULL does not
    assert l.lwkzg_recover_cells_and_kzg_proofs_mixed(None, None, None, None, None, 0, ps, None) == K.C_KZG_OK
    assert l.lwkzg_recover_cells_and_kzg_proofs_mixed_device(None, None, None, None, None, 0, ps, None, None) == K.C_KZG_OK
    assert both([a, b, a], n_blobs=0) == [(K.C_KZG_OK, untouched), (K.C_KZG_OK, None)]
    assert l.lwkzg_recover_cells_and_kzg_proofs_mixed(None, None, None, None, None, 0, None, None) == K.C_KZG_BADARGS
    assert l.lwkzg_recover_cells_and_kzg_proofs_mixed_device(None, None, None, None, None, 0, None, None, None) == K.C_KZG_BADARGS
    # what is wrong with the call as a whole names no blob
    assert both([a, b, a], settings=None) == refused(untouched)
    assert both([a, b, a], indices=False) == refused(untouched)
    assert both([a, b, a], cells=False) == refused(untouched)
    assert both([a, b, a], counts=False) == refused(untouched)
    assert both([a, b, a], out=(None, None)) == refused(untouched)
    # a list at fault names its blob: in front, in the middle, at the end
    faulty = {
        "count 63": a[:63],
        "count 129": list(range(129)),
        "count 0": [],
        "index 128": a[:63] + [128],
        "index 2^64 - 1": a[:63] + [2 ** 64 - 1],
        "a repeated index": a[:10] + [9] + a[11:],
        "a descending pair": a[:10] + [11, 10] + a[12:],
        "descending": list(range(1, 65))[::-1],
    }
    for name, lst in faulty.items():
        for at in range(3):
            lists = [a, b, a]
            lists[at] = lst
            assert both(lists) == refused(at), (name, at)
    # the first faulty list is the one that is named
    assert both([a, faulty["index 128"], faulty["count 63"]]) == refused(1)
    assert cells_out.raw == bytes(n * 128 * 2048) and proofs.raw == bytes(n * 128 * 48)
    # in c-kzg mode the same code
    prev = K.set_mode(K.MODE_CKZG)
    try:
        assert both([a, faulty["count 63"]]) == refused(1) and both([faulty["index 128"], b]) == refused(0)
        assert both([a, b], counts=False) == refused(untouched)
    finally:
        K.set_mode(prev)
