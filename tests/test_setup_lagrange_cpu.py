"""CPU: the Lagrange-form fixture (a c-kzg-4844 1.x layout of the tau = 1337 setup; tests/golden/make_lagrange_setup.py writes it, pinned
by size and SHA-256) against the oracle, the integer identity the device derivation rests on, and everything the c-kzg loaders decide before any
device work."""
import ctypes as C
import os
import re

import pytest

import make_lagrange_setup as L
from conftest import R, ROOT, SETUP_PATH, TAU

NEW_SYMBOLS = ["lwkzg_load_trusted_setup_lagrange", "lwkzg_load_trusted_setup_ckzg", "lwkzg_load_trusted_setup_file_ckzg",
               "lwkzg_setup_g1_lagrange", "lwkzg_trusted_setup_check"]


@pytest.fixture(scope="module")
def lagrange_path(tmp_path_factory, oracle):
    """the Lagrange text, generated once (make_lagrange_setup.write checks its pinned size and digest)"""
    return L.write(str(tmp_path_factory.mktemp("lagrange_setup")))


@pytest.fixture(scope="module")
def tokens(lagrange_path):
    with open(lagrange_path) as f:
        return f.read().split()


@pytest.fixture(scope="module")
def scalars():
    return L.lagrange_scalars(TAU)


def test_fixture_layout_and_size(tokens, lagrange_path):
    assert os.path.getsize(lagrange_path) == 409864 == os.path.getsize(SETUP_PATH) == L.SIZE
    assert tokens[:2] == ["4096", "65"] and len(tokens) == 2 + 4096 + 65
    assert all(len(t) == 96 for t in tokens[2:2 + 4096]) and all(len(t) == 192 for t in tokens[2 + 4096:])


def test_sampled_points_match_the_oracle(tokens, scalars, oracle):
    sample = [0, 1, 2, 3, 64, 1023, 1024, 2047, 2048, 2049, 3071, 3072, 4000, 4093, 4094, 4095]
    assert len(sample) == 16
    for i in sample:
        want = (TAU ** 4096 - 1) * pow(4096, -1, R) * pow(L.OMEGA, i, R) * pow(TAU - pow(L.OMEGA, i, R), -1, R) % R
        assert scalars[i] == want, i
        assert bytes.fromhex(tokens[2 + i]) == oracle.g1_generator_mul(want), i
    assert L.g1_points(scalars, sample) == [bytes.fromhex(tokens[2 + i]) for i in sample]


def test_forward_dft_of_the_lagrange_scalars_gives_the_powers_of_tau(scalars):
    """sum_i w^(i j) l_i(tau) = tau^j: row j of the forward DFT matrix over the Lagrange form is the monomial point j (k_dft_rows)"""
    assert pow(L.OMEGA, 4096, R) == 1 and pow(L.OMEGA, 2048, R) == R - 1
    for j in (0, 1, 2, 63, 2048, 4095):
        assert sum(pow(L.OMEGA, i * j, R) * s for i, s in enumerate(scalars)) % R == pow(TAU, j, R), j
    # the same through the inverse transform the tests use for setups that are no powers of anything
    assert L.lagrange_scalars_of([pow(TAU, j, R) for j in range(4096)]) == scalars


def test_g2_lines_are_those_of_the_monomial_fixture(tokens):
    with open(SETUP_PATH) as f:
        mono = f.read().split()
    assert tokens[2 + 4096:] == mono[2 + 4096:]
    assert tokens[2:2 + 4096] != mono[2:2 + 4096] and tokens[2] != mono[2]   # (l_0(tau) G is not the generator)


def test_new_symbols_are_declared_exported_and_bound(K):
    from lambdaworks_kzg_amd import capi
    header = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    l = K.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bC_KZG_RET %s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(l, name), name
    for method in ("from_lagrange_bytes", "from_ckzg_bytes", "from_ckzg_file", "g1_lagrange", "check"):
        assert hasattr(K.TrustedSetup, method), method


def _sentinel_settings(K):
    s = K.KZGSettings()
    s.fs, s.g1_values, s.g2_values = 0x1111, 0x2222, 0x3333
    return s


def _untouched(s):
    return (s.fs, s.g1_values, s.g2_values) == (0x1111, 0x2222, 0x3333)


def test_bad_arguments_of_the_byte_loaders_need_no_gpu(K):
    l = K.lib()
    s = _sentinel_settings(K)
    g1, g2 = b"\0" * (4096 * 48), b"\0" * (65 * 96)
    B = K.C_KZG_BADARGS
    assert l.lwkzg_load_trusted_setup_lagrange(None, g1, 4096, g2, 65) == B
    assert l.lwkzg_load_trusted_setup_lagrange(C.byref(s), None, 4096, g2, 65) == B
    assert l.lwkzg_load_trusted_setup_lagrange(C.byref(s), g1, 4096, None, 65) == B
    assert l.lwkzg_load_trusted_setup_lagrange(C.byref(s), g1, 4095, g2, 65) == B
    assert l.lwkzg_load_trusted_setup_lagrange(C.byref(s), g1, 4096, g2, 64) == B
    assert l.lwkzg_load_trusted_setup_lagrange(C.byref(s), g1, 0, g2, 0) == B
    assert l.lwkzg_load_trusted_setup_ckzg(None, g1, 4096, g1, 4096, g2, 65, 0) == B
    assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), None, 4096, g1, 4096, g2, 65, 0) == B
    assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), g1, 4096, None, 4096, g2, 65, 0) == B
    assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), g1, 4096, g1, 4096, None, 65, 0) == B
    assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), g1, 4095, g1, 4096, g2, 65, 0) == B
    assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), g1, 4096, g1, 8192, g2, 65, 0) == B
    assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), g1, 4096, g1, 4096, g2, 66, 8) == B
    assert l.lwkzg_load_trusted_setup_file_ckzg(None, None) == B
    assert l.lwkzg_load_trusted_setup_file_ckzg(C.byref(s), None) == B
    assert l.lwkzg_setup_g1_lagrange(None, C.byref(s)) == B
    assert l.lwkzg_setup_g1_lagrange(C.create_string_buffer(4096 * 48), None) == B
    ok = C.c_bool(True)
    assert l.lwkzg_trusted_setup_check(None, C.byref(s)) == B
    assert l.lwkzg_trusted_setup_check(C.byref(ok), None) == B
    empty = K.KZGSettings()
    assert l.lwkzg_trusted_setup_check(C.byref(ok), C.byref(empty)) == B and ok.value is False
    assert _untouched(s)


def _load_text(K, tmp_path, text, name="setup.txt"):
    from lambdaworks_kzg_amd import capi
    path = tmp_path / name
    path.write_bytes(text if isinstance(text, bytes) else text.encode())
    s = _sentinel_settings(K)
    fp = capi._libc.fopen(os.fsencode(str(path)), b"r")
    assert fp
    try:
        rc = K.lib().lwkzg_load_trusted_setup_file_ckzg(C.byref(s), fp)
    finally:
        capi._libc.fclose(fp)
    assert _untouched(s)
    return rc, K.lib().lwkzg_last_error().decode()


def test_bad_texts_are_badargs_without_a_gpu(K, tmp_path, tokens):
    B = K.C_KZG_BADARGS
    assert _load_text(K, tmp_path, "")[0] == B
    assert _load_text(K, tmp_path, "4096\n")[0] == B
    assert _load_text(K, tmp_path, "\n".join(["4095"] + tokens[1:]))[0] == B
    assert _load_text(K, tmp_path, "\n".join(["99999999999999999999"] + tokens[1:]))[0] == B
    # a token count that fits neither layout: one point short, one too many, a section and a half
    rc, err = _load_text(K, tmp_path, "\n".join(tokens[:-1]))
    assert rc == B and "neither layout" in err
    rc, err = _load_text(K, tmp_path, "\n".join(tokens + [tokens[2]]))
    assert rc == B and "neither layout" in err
    rc, err = _load_text(K, tmp_path, "\n".join(tokens + tokens[2:2 + 2048]))
    assert rc == B and "neither layout" in err
    # a token that is not hex, in each section of the three-section layout
    three = tokens + tokens[2:2 + 4096]
    for at, what in ((2 + 5, "g1 lagrange point 5"), (2 + 4096 + 64, "g2 point 64"), (2 + 4096 + 65 + 4095, "g1 monomial point 4095")):
        bad = list(three)
        bad[at] = bad[at][:10] + "x" + bad[at][11:]
        rc, err = _load_text(K, tmp_path, "\n".join(bad))
        assert rc == B and what in err and "not hex" in err, err
    # a token of the wrong length: cut by two characters, and a file that ends in the middle of a token
    bad = list(tokens)
    bad[2 + 100] = bad[2 + 100][:-2]
    rc, err = _load_text(K, tmp_path, "\n".join(bad))
    assert rc == B and "g1 lagrange point 100 has 94 characters" in err
    rc, err = _load_text(K, tmp_path, "\n".join(tokens)[:-7])
    assert rc == B and "g2 point 64 has 185 characters" in err


def test_a_well_formed_file_fails_without_a_gpu_as_the_monomial_loader_does(K, tmp_path, tokens, lagrange_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(K.KzgError) as e:
        K.TrustedSetup.from_file(SETUP_PATH)
    want = e.value.rc
    assert want == K.C_KZG_ERROR
    for text in ("\n".join(tokens), " ".join(tokens), "\r\n".join(tokens + tokens[2:2 + 4096]) + "\r\n"):
        rc, err = _load_text(K, tmp_path, text)
        assert rc == want and "no CPU fallback" in err
    with pytest.raises(K.KzgError) as e:
        K.TrustedSetup.from_ckzg_file(lagrange_path)
    assert e.value.rc == want
    g1 = b"".join(bytes.fromhex(t) for t in tokens[2:2 + 4096])
    g2 = b"".join(bytes.fromhex(t) for t in tokens[2 + 4096:])
    with pytest.raises(K.KzgError) as e:
        K.TrustedSetup.from_lagrange_bytes(g1, g2)
    assert e.value.rc == want
    with pytest.raises(K.KzgError) as e:
        K.TrustedSetup.from_ckzg_bytes(g1, g1, g2)
    assert e.value.rc == want
