"""GPU: c-kzg-4844 trusted setups -- G1 in LAGRANGE form, natural order -- through lwkzg_load_trusted_setup_lagrange (c-kzg 1.x: the
monomial points are derived on the device, 4096 MSMs of forward-DFT rows over the Lagrange points), lwkzg_load_trusted_setup_ckzg (c-kzg
2.x: both sections given, validated and held against each other) and lwkzg_load_trusted_setup_file_ckzg (either text layout), with
lwkzg_setup_g1_lagrange (the way back out) and lwkzg_trusted_setup_check (is this a powers-of-tau setup?).

The yardstick is the monomial load of the same setup (load_trusted_setup_file on tests/golden/trusted_setup*.txt): the settings must be
indistinguishable from it -- g1_values and g2_values byte for byte, every answer the same on the bucket engine and on a direct table, in
c-kzg mode and in reference mode -- for tau = 1337, a 255-bit tau' and a setup that is no powers of anything. The Lagrange bytes of the
first are the text tests/golden/make_lagrange_setup.py writes (pinned by digest); those of the other two are computed here by the same functions
and the CPU oracle."""
import ctypes as C
import os

import pytest

import blobs as B
import make_lagrange_setup as L
import make_setups as M
from conftest import P, SETUP_PATH, SETUP_TAU2_PATH, SETUP_UNSTRUCTURED_PATH, hx

pytestmark = pytest.mark.gpu

N1, N2 = 4096, 65


def _sections(path):
    with open(path) as f:
        t = f.read().split()
    assert t[:2] == ["4096", "65"] and len(t) == 2 + N1 + N2
    return t[2:2 + N1], t[2 + N1:]


def _join(hex_tokens):
    return b"".join(bytes.fromhex(x) for x in hex_tokens)


@pytest.fixture(scope="module")
def lagrange_path(tmp_path_factory, oracle):
    """the c-kzg 1.x text of the tau = 1337 setup, generated once (make_lagrange_setup.write checks its pinned size and digest)"""
    return L.write(str(tmp_path_factory.mktemp("lagrange_setup")))


@pytest.fixture(scope="module")
def setups(oracle, lagrange_path):
    """name -> (path of the monomial text, g1 monomial bytes, g1 Lagrange bytes in natural order, g2 bytes), computed once"""
    out = {}
    lag_1337, g2_1337 = _sections(lagrange_path)
    for name, path in (("tau1337", SETUP_PATH), ("tau2", SETUP_TAU2_PATH), ("unstructured", SETUP_UNSTRUCTURED_PATH)):
        g1, g2 = _sections(path)
        if name == "tau1337":
            assert g2 == g2_1337
            lag = _join(lag_1337)
        elif name == "tau2":
            lag = b"".join(L.g1_points(L.lagrange_scalars(M.TAU2)))
        else:
            lag = b"".join(L.g1_points(L.lagrange_scalars_of([M.unstructured_scalar(j) for j in range(N1)])))
        out[name] = (path, _join(g1), lag, _join(g2))
    return out


@pytest.fixture(autouse=True)
def _reference_default(K):
    K.set_mode(K.MODE_REFERENCE)   # the process default: the c-kzg loaders must not depend on it
    yield
    K.set_mode(K.MODE_REFERENCE)


def _sentinel(K):
    s = K.KZGSettings()
    s.fs, s.g1_values, s.g2_values = 0x1111, 0x2222, 0x3333
    return s


def _untouched(s):
    return (s.fs, s.g1_values, s.g2_values) == (0x1111, 0x2222, 0x3333)


def _err(K):
    return K.lib().lwkzg_last_error().decode()


def _three_section_text(setups, name, sep="\n"):
    _, mono, lag, g2 = setups[name]
    tok = ["4096", "65"] + [lag[48 * i:48 * i + 48].hex() for i in range(N1)] + [g2[96 * i:96 * i + 96].hex() for i in range(N2)] + \
          [mono[48 * i:48 * i + 48].hex() for i in range(N1)]
    return sep.join(tok)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tau1337", "tau2", "unstructured"])
def test_lagrange_load_equals_the_monomial_load(K, setups, name):
    path, mono_bytes, lag, g2 = setups[name]
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_lagrange_bytes(lag, g2)
    mono = K.TrustedSetup.from_file(path)
    try:
        assert ts.get_mode() == K.MODE_CKZG and mono.get_mode() == K.MODE_REFERENCE and K.get_mode() == K.MODE_REFERENCE
        g1v = ts.g1_values_bytes()
        assert len(g1v) == N1 * 144 and g1v == mono.g1_values_bytes()
        assert ts.g2_values_bytes() == mono.g2_values_bytes()
        assert ts.fft_settings().max_width == 4096
        assert ts.g1_lagrange() == lag                 # the input, as given
        assert mono.g1_lagrange() == lag               # and the form a monomial load derives is the same one
        assert mono.get_mode() == K.MODE_REFERENCE     # (asking for it changes no mode)
        rep = ts.timing_report()["load"]
        assert rep["derive_monomial_ms"] > 0 and rep["cross_check_ms"] == 0 and rep["lagrange_section_ms"] > 0
    finally:
        ts.free()
        mono.free()


# ---- 2. same answers as a monomial load switched to c-kzg mode ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair(K, setups):
    """(Lagrange-loaded, monomial-loaded) settings of the tau = 1337 setup"""
    _, _, lag, g2 = setups["tau1337"]
    ts = K.TrustedSetup.from_lagrange_bytes(lag, g2)
    mono = K.TrustedSetup.from_file(SETUP_PATH)
    yield ts, mono
    ts.free()
    mono.free()


def _answers(K, ts, le):
    blobs = [B.synthetic_blob(7000 + i, big_endian=not le) for i in range(3)]
    out = {}
    out["commit1"] = K.blob_to_kzg_commitment_batch(blobs[0], ts)
    out["commit3"] = K.blob_to_kzg_commitment_batch(b"".join(blobs), ts)
    out["proof"] = K.compute_blob_kzg_proof(blobs[1], out["commit3"][1], ts)
    out["verify"] = K.verify_blob_kzg_proof(blobs[1], out["commit3"][1], out["proof"], ts)
    out["verify_wrong"] = K.verify_blob_kzg_proof(blobs[1], out["commit3"][2], out["proof"], ts)
    cells, proofs = K.compute_cells_and_kzg_proofs(blobs[2], ts)
    out["cells"], out["cell_proofs"] = b"".join(cells), b"".join(proofs)
    return out


def _first_good(vectors, suite):
    for c in vectors["suites"][suite]:
        if c["output"] not in (None, False):
            return c
    raise AssertionError(suite)


@pytest.mark.parametrize("bits", [0, 10])
def test_answers_equal_those_of_a_monomial_load(K, pair, vectors, bits):
    ts, mono = pair
    ts.enable_direct_table(bits)
    mono.enable_direct_table(bits)
    assert ts.direct_table_bits() == bits == mono.direct_table_bits()
    assert ts.get_mode() == K.MODE_CKZG
    mono.set_mode(K.MODE_CKZG)
    try:
        got, want = _answers(K, ts, True), _answers(K, mono, True)
        assert got == want and got["verify"] is True and got["verify_wrong"] is False
        assert len(got["commit3"]) == 3 and len(got["cell_proofs"]) == 128 * 48
        # one c-kzg vector per suite
        c = _first_good(vectors, "blob_to_kzg_commitment")
        assert K.blob_to_kzg_commitment(B.make_blob(c["input"]["blob"]), ts) == hx(c["output"])
        c = _first_good(vectors, "compute_kzg_proof")
        pr, y = K.compute_kzg_proof(B.make_blob(c["input"]["blob"]), hx(c["input"]["z"]), ts)
        assert (pr, y) == (hx(c["output"][0]), hx(c["output"][1]))
        c = _first_good(vectors, "compute_blob_kzg_proof")
        assert K.compute_blob_kzg_proof(B.make_blob(c["input"]["blob"]), hx(c["input"]["commitment"]), ts) == hx(c["output"])
        c = _first_good(vectors, "verify_kzg_proof")
        assert K.verify_kzg_proof(hx(c["input"]["commitment"]), hx(c["input"]["z"]), hx(c["input"]["y"]), hx(c["input"]["proof"]), ts) is True
        c = _first_good(vectors, "verify_blob_kzg_proof")
        assert K.verify_blob_kzg_proof(B.make_blob(c["input"]["blob"]), hx(c["input"]["commitment"]), hx(c["input"]["proof"]), ts) is True
        c = _first_good(vectors, "verify_blob_kzg_proof_batch")
        n = len(c["input"]["blobs"])
        assert K.verify_blob_kzg_proof_batch(b"".join(B.make_blob(b) for b in c["input"]["blobs"]), b"".join(hx(x) for x in c["input"]["commitments"]),
                                             b"".join(hx(x) for x in c["input"]["proofs"]), n, ts) is True
        # and in reference mode, after lwkzg_settings_set_mode
        assert ts.set_mode(K.MODE_REFERENCE) == K.MODE_CKZG
        mono.set_mode(K.MODE_REFERENCE)
        got, want = _answers(K, ts, False), _answers(K, mono, False)
        assert got == want and got["verify"] is True and got["verify_wrong"] is False
    finally:
        ts.set_mode(K.MODE_CKZG)
        mono.set_mode(-1)


# ---- 3. the file loader ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spacing", ["as_written", "single_spaces"])
@pytest.mark.parametrize("layout", ["one_section", "three_sections"])
def test_file_loader_takes_both_layouts_and_any_whitespace(K, setups, pair, lagrange_path, tmp_path, layout, spacing):
    _, _, lag, g2 = setups["tau1337"]
    loaded, mono = pair
    if layout == "one_section":
        with open(lagrange_path) as f:   # the generated text as it is
            text = f.read()
    else:
        text = _three_section_text(setups, "tau1337") + "\n"
    if spacing == "single_spaces":       # one line, as c-kzg's fscanf accepts
        text = " ".join(text.split())
    path = tmp_path / "setup.txt"
    path.write_text(text)
    blob = B.synthetic_blob(7100, big_endian=False)
    ts = K.TrustedSetup.from_ckzg_file(str(path))
    try:
        assert ts.get_mode() == K.MODE_CKZG
        assert ts.g1_values_bytes() == mono.g1_values_bytes() and ts.g2_values_bytes() == mono.g2_values_bytes()
        assert ts.g1_lagrange() == lag
        rep = ts.timing_report()["load"]
        assert (rep["derive_monomial_ms"] > 0) == (layout == "one_section") and (rep["cross_check_ms"] > 0) == (layout == "three_sections")
        assert loaded.get_mode() == K.MODE_CKZG
        assert K.blob_to_kzg_commitment(blob, ts) == K.blob_to_kzg_commitment(blob, loaded)
    finally:
        ts.free()


# ---- 4. the three-section form fails closed ----------------------------------------------------------------------------------------

def _swap48(data, i, j):
    b = bytearray(data)
    b[48 * i:48 * i + 48], b[48 * j:48 * j + 48] = data[48 * j:48 * j + 48], data[48 * i:48 * i + 48]
    return bytes(b)


def _brp(i):
    return int(format(i, "012b")[::-1], 2)


def test_three_section_form_fails_closed(K, setups):
    _, mono, lag, g2 = setups["tau1337"]
    l = K.lib()
    cases = {
        "two Lagrange points swapped": (mono, _swap48(lag, 17, 3000), g2),
        "a monomial point replaced by another point of the subgroup": (mono[:48 * 5] + mono[48 * 6:48 * 7] + mono[48 * 6:], lag, g2),
        "the Lagrange section in bit-reversed order": (mono, b"".join(lag[48 * _brp(i):48 * _brp(i) + 48] for i in range(N1)), g2),
        "the monomial section of another setup": (setups["tau2"][1], lag, g2),
    }
    for what, (m, lg, g) in cases.items():
        s = _sentinel(K)
        rc = l.lwkzg_load_trusted_setup_ckzg(C.byref(s), m, N1, lg, N1, g, N2, 0)
        assert rc == K.C_KZG_BADARGS, what
        assert "not the same setup" in _err(K), what
        assert _untouched(s), what
    ts = K.TrustedSetup.from_ckzg_bytes(mono, lag, g2, precompute=8)
    try:
        rep = ts.timing_report()["load"]
        assert rep["derive_monomial_ms"] == 0 and rep["cross_check_ms"] > 0      # nothing was derived
        assert ts.get_mode() == K.MODE_CKZG and ts.g1_lagrange() == lag
        ref = K.TrustedSetup.from_file(SETUP_PATH)
        assert ts.g1_values_bytes() == ref.g1_values_bytes() and ts.g2_values_bytes() == ref.g2_values_bytes()
        ref.free()
    finally:
        ts.free()


# ---- 5. bad points -----------------------------------------------------------------------------------------------------------------

def _g1_x(on_curve):
    """a compressed G1 encoding whose x is (is not) the abscissa of a curve point; such a point is outside the subgroup (cofactor ~2^125)"""
    x = 5
    while (pow((x ** 3 + 4) % P, (P - 1) // 2, P) == 1) != on_curve:
        x += 1
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80
    return bytes(b)


BAD_POINTS = {"off the curve": lambda: _g1_x(False), "outside the subgroup": lambda: _g1_x(True), "infinity": lambda: bytes([0xC0]) + bytes(47)}


@pytest.mark.parametrize("kind", list(BAD_POINTS))
def test_bad_points_are_badargs_with_their_index(K, setups, kind):
    _, mono, lag, g2 = setups["tau1337"]
    l = K.lib()
    bad = BAD_POINTS[kind]()
    word = "infinity" if kind == "infinity" else "invalid compressed point or not in the subgroup"

    def put(data, i):
        return data[:48 * i] + bad + data[48 * i + 48:]

    for i in (0, 1, 2049, 4095):   # (natural indices: the caller's, not the permuted ones)
        s = _sentinel(K)
        assert l.lwkzg_load_trusted_setup_lagrange(C.byref(s), put(lag, i), N1, g2, N2) == K.C_KZG_BADARGS
        assert "g1 lagrange point %d" % i in _err(K) and word in _err(K) and _untouched(s)
    for i in (0, 4095):
        s = _sentinel(K)
        assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), mono, N1, put(lag, i), N1, g2, N2, 0) == K.C_KZG_BADARGS
        assert "g1 lagrange point %d" % i in _err(K) and word in _err(K) and _untouched(s)
        assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), put(mono, i), N1, lag, N1, g2, N2, 0) == K.C_KZG_BADARGS
        assert "g1 monomial point %d" % i in _err(K) and word in _err(K) and _untouched(s)


def test_bad_g2_point_is_badargs(K, setups):
    _, mono, lag, g2 = setups["tau1337"]
    l = K.lib()
    bad = bytearray(g2)
    bad[96 * 40] &= 0x7F   # not a compressed encoding
    s = _sentinel(K)
    assert l.lwkzg_load_trusted_setup_lagrange(C.byref(s), lag, N1, bytes(bad), N2) == K.C_KZG_BADARGS
    assert "g2 point 40" in _err(K) and _untouched(s)
    assert l.lwkzg_load_trusted_setup_ckzg(C.byref(s), mono, N1, lag, N1, bytes(bad), N2, 0) == K.C_KZG_BADARGS
    assert "g2 point 40" in _err(K) and _untouched(s)


# ---- 6. lwkzg_trusted_setup_check -------------------------------------------------------------------------------------------------

LOADERS = ["load_trusted_setup_file", "load_trusted_setup", "lagrange bytes", "c-kzg bytes", "c-kzg file, one section", "c-kzg file, three sections"]


@pytest.mark.parametrize("loader", LOADERS)
@pytest.mark.parametrize("name", ["tau1337", "tau2"])
def test_check_accepts_powers_of_tau_through_every_loader(K, setups, tmp_path, name, loader):
    path, mono, lag, g2 = setups[name]
    if loader == "load_trusted_setup_file":
        ts = K.TrustedSetup.from_file(path)
    elif loader == "load_trusted_setup":
        ts = K.TrustedSetup.from_bytes(mono, g2)
    elif loader == "lagrange bytes":
        ts = K.TrustedSetup.from_lagrange_bytes(lag, g2)
    elif loader == "c-kzg bytes":
        ts = K.TrustedSetup.from_ckzg_bytes(mono, lag, g2)
    else:
        text = tmp_path / "setup.txt"
        if loader == "c-kzg file, three sections":
            text.write_text(_three_section_text(setups, name))
        else:
            text.write_text("\n".join(["4096", "65"] + [lag[48 * i:48 * i + 48].hex() for i in range(N1)] + [g2[96 * i:96 * i + 96].hex() for i in range(N2)]))
        ts = K.TrustedSetup.from_ckzg_file(str(text))
    try:
        before = (ts.g1_values_bytes(), ts.g2_values_bytes(), ts.get_mode(), ts.direct_table_bits(), ts.direct_table_forms())
        assert ts.check() is True
        assert before == (ts.g1_values_bytes(), ts.g2_values_bytes(), ts.get_mode(), ts.direct_table_bits(), ts.direct_table_forms())
        if loader == "lagrange bytes":   # and on the bucket engine
            ts.enable_direct_table(0)
            assert ts.check() is True
    finally:
        ts.free()


NOT_POWERS_OF_TAU = ["the unstructured setup", "the unstructured setup from its Lagrange bytes", "g2[2] and g2[3] swapped",
                     "the trap: a Lagrange file read as monomial", "the trap from bytes", "monomial bytes handed to the Lagrange loader",
                     "two monomial points swapped", "the G2 half of another tau"]


@pytest.mark.parametrize("what", NOT_POWERS_OF_TAU)
def test_check_rejects_what_is_no_powers_of_tau(K, setups, lagrange_path, what):
    _, mono, lag, g2 = setups["tau1337"]
    upath, umono, ulag, ug2 = setups["unstructured"]
    g2_swapped = g2[:96 * 2] + g2[96 * 3:96 * 4] + g2[96 * 2:96 * 3] + g2[96 * 4:]
    loaders = {
        "the unstructured setup": lambda: K.TrustedSetup.from_file(upath),
        "the unstructured setup from its Lagrange bytes": lambda: K.TrustedSetup.from_lagrange_bytes(ulag, ug2),
        "g2[2] and g2[3] swapped": lambda: K.TrustedSetup.from_bytes(mono, g2_swapped),
        "the trap: a Lagrange file read as monomial": lambda: K.TrustedSetup.from_file(lagrange_path),
        "the trap from bytes": lambda: K.TrustedSetup.from_bytes(lag, g2),
        "monomial bytes handed to the Lagrange loader": lambda: K.TrustedSetup.from_lagrange_bytes(mono, g2),
        "two monomial points swapped": lambda: K.TrustedSetup.from_bytes(_swap48(mono, 100, 101), g2),
        "the G2 half of another tau": lambda: K.TrustedSetup.from_bytes(mono, setups["tau2"][3]),
    }
    assert sorted(loaders) == sorted(NOT_POWERS_OF_TAU)
    ts = loaders[what]()
    try:
        assert ts.check() is False
    finally:
        ts.free()


# ---- 7. the setup image ------------------------------------------------------------------------------------------------------------

def test_setup_image_of_a_lagrange_loaded_setup(K, pair):
    import torch
    from lambdaworks_kzg_amd import capi
    ts, _ = pair
    img = torch.empty(capi.setup_image_bytes(), dtype=torch.uint8, device="cuda")
    ts.export_device_image(img.data_ptr())
    torch.cuda.synchronize()
    imp = K.TrustedSetup.from_device_image(img.data_ptr())
    try:
        imp.enable_direct_table(0)
        assert imp.g1_values_bytes() == ts.g1_values_bytes() and imp.g2_values_bytes() == ts.g2_values_bytes()
        for mode, le in ((K.MODE_CKZG, True), (K.MODE_REFERENCE, False)):
            blob = B.synthetic_blob(7200, big_endian=not le)
            ts.set_mode(mode)
            imp.set_mode(mode)
            assert K.blob_to_kzg_commitment(blob, imp) == K.blob_to_kzg_commitment(blob, ts)
        assert imp.g1_lagrange() == ts.g1_lagrange()
    finally:
        ts.set_mode(K.MODE_CKZG)
        imp.free()


# ---- 8. memory ---------------------------------------------------------------------------------------------------------------------

def test_load_and_free_leave_nothing_behind(K, setups):
    import torch
    _, mono, lag, g2 = setups["tau1337"]
    blob = B.synthetic_blob(7300, big_endian=False)
    free_after = []
    for k in range(4):
        ts = K.TrustedSetup.from_lagrange_bytes(lag, g2) if k % 2 == 0 else K.TrustedSetup.from_ckzg_bytes(mono, lag, g2)
        K.blob_to_kzg_commitment(blob, ts)
        ts.free()
        torch.cuda.synchronize()
        free_after.append(torch.cuda.mem_get_info()[0])
    assert free_after[1] == free_after[3], free_after   # (the first cycles may still grow the runtime's own pools)
    # a failed load keeps nothing either
    s = _sentinel(K)
    assert K.lib().lwkzg_load_trusted_setup_ckzg(C.byref(s), mono, N1, _swap48(lag, 1, 2), N1, g2, N2, 0) == K.C_KZG_BADARGS
    assert K.lib().lwkzg_load_trusted_setup_lagrange(C.byref(s), lag[:48] + bytes([0xC0]) + bytes(47) + lag[96:], N1, g2, N2) == K.C_KZG_BADARGS
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free_after[3] and _untouched(s)
