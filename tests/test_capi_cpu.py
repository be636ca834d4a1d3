"""CPU: the C-ABI library loads, exports every symbol include/lambdaworks_kzg_amd.h declares, has the
reference's struct layouts, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, SETUP_PATH


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "lambdaworks_kzg_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(?:C_KZG_RET|int|size_t|void|const char \*|const KZGSettings \*)\s*\*?\s*([a-z_0-9]+)\s*\(", src)
    return sorted(set(n for n in names if n not in ("defined",)))


def test_header_and_binding_agree(K):
    from lambdaworks_kzg_amd import capi
    declared = _declared_functions()
    assert len(declared) >= 30
    assert sorted(capi.EXPORTED_SYMBOLS) == declared


def test_library_exports_every_declared_symbol(K):
    l = K.lib()
    for name in _declared_functions():
        assert hasattr(l, name), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "lambdaworks_kzg_amd", "lib",
                                                                              "liblambdaworks_kzg.so")]).decode()
    exported = set(re.findall(r" T ([A-Za-z_0-9]+)", out))
    assert set(_declared_functions()) <= exported
    # and nothing else is exported: the nine reference symbols + lwkzg_* (csrc/exports.map; VERDICT r03 found a kernel stub among them)
    every = set(re.findall(r" [A-Za-z] ([A-Za-z_0-9$.]+)", out))
    stray = sorted(n for n in every if n not in set(_declared_functions()))
    assert not stray, stray
    # nothing of the oracle leaks into the product
    assert not any(s.startswith("orc_") for s in exported)


def test_product_does_not_reference_oracle():
    pkg = os.path.join(ROOT, "lambdaworks_kzg_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".h", ".cpp")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert "oracle" not in txt.replace("TEST INFRASTRUCTURE", ""), os.path.join(dp, f)


def test_header_compiles_as_c_and_layouts_match_reference(tmp_path):
    # sizes from /root/reference/src/lib.rs:103-232 (blst_p1 144 B, blst_p2 288 B, Blob 131072 B, three pointers)
    src = tmp_path / "t.c"
    src.write_text('#include "lambdaworks_kzg_amd.h"\n#include <stdio.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(blst_fp), sizeof(blst_p1),'
                   'sizeof(blst_p2), sizeof(Blob), sizeof(KZGSettings), sizeof(FFTSettings), sizeof(Bytes48),'
                   '(int)C_KZG_MALLOC);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"48", b"144", b"288", b"131072", b"24", b"32", b"48", b"3"]


def test_mode_switch(K):
    prev = K.set_mode(K.MODE_CKZG)
    assert K.get_mode() == K.MODE_CKZG
    assert K.set_mode(7) == -1 and K.get_mode() == K.MODE_CKZG
    K.set_mode(prev)
    assert K.get_mode() == prev


def test_argument_checks_need_no_gpu(K):
    l = K.lib()
    s = K.KZGSettings()
    # lib.rs:716-718: wrong counts are the reference's only BADARGS
    assert l.load_trusted_setup(C.byref(s), b"\0" * 48, 1, b"\0" * 96, 1) == K.C_KZG_BADARGS
    ok = C.c_bool(True)
    # lib.rs:538-543: n == 0 -> OK with ok = false
    assert l.verify_blob_kzg_proof_batch(C.byref(ok), None, None, None, 0, C.byref(s)) == K.C_KZG_OK
    assert ok.value is False
    # the node-level entry points (csrc/multi.hip): no handle, no devices, a device that is not there
    h = C.c_void_p(1)
    assert l.lwkzg_multi_load(C.byref(h), b"", 0, b"", 0, None, 0) == K.C_KZG_BADARGS and not h.value
    one = (C.c_int * 1)(4096)
    assert l.lwkzg_multi_load(C.byref(h), b"", 0, b"", 0, one, 1) == K.C_KZG_BADARGS and b"visible" in l.lwkzg_last_error()
    assert l.lwkzg_multi_device_count(None) == 0 and l.lwkzg_multi_device(None, 0) == -1 and not l.lwkzg_multi_settings(None, 0)
    assert l.lwkzg_multi_blob_to_kzg_commitment_batch(None, None, 0, None, None) == K.C_KZG_BADARGS
    assert l.lwkzg_multi_verify_blob_kzg_proof_batch(C.byref(ok), None, None, None, 0, None) == K.C_KZG_BADARGS and ok.value is False
    l.lwkzg_multi_free(None)


def test_fails_loudly_without_gpu(K):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(K.KzgError) as e:
        K.TrustedSetup.from_file(SETUP_PATH)
    assert e.value.rc == K.C_KZG_ERROR and "no CPU fallback" in str(e.value)


def test_host_pairing_product(K, oracle, oracle_setup):
    """verify side, host only: e(G, [tau]G2) * e(-[tau]G, G2) == 1 for the tau = 1337 setup, and negatives."""
    from lambdaworks_kzg_amd import capi
    g1, g2 = oracle_setup.g1_compressed(), oracle_setup.g2_compressed()
    G, tG, H, tH = g1[:48], g1[48:96], g2[:96], g2[96:192]

    def negc(c):
        b = bytearray(c)
        b[0] ^= 0x20          # flip the ZCash sign bit: -P
        return bytes(b)

    assert capi.pairing_product_is_one(G + negc(tG), tH + H) is True
    assert capi.pairing_product_is_one(G + negc(G), tH + H) is False
    assert capi.pairing_product_is_one(oracle.g1_generator_mul(5) + negc(oracle.g1_generator_mul(5 * 1337)), tH + H) is True
    assert capi.pairing_product_is_one(G, H) is False
    assert capi.pairing_product_is_one(bytes([0xc0]) + bytes(47), H) is True      # e(O, Q) = 1


_PAIRING_CASES = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from lambdaworks_kzg_amd import capi
lines = open(%r).read().split()
g1 = [bytes.fromhex(x) for x in lines[2:2 + 4096]]
g2 = [bytes.fromhex(x) for x in lines[2 + 4096:2 + 4096 + 65]]
def negc(c):
    b = bytearray(c); b[0] ^= 0x20; return bytes(b)
out = []
for j, k in [(0, 1), (3, 2), (5, 7), (1, 11), (9, 13), (2, 17), (4, 19), (6, 23), (8, 29), (10, 31), (12, 37), (0, 64)]:
    # e([tau^j]G, [tau^k]H) * e(-[tau^(j+k)]G, H) == 1; twelve distinct first G2 points (more than the line cache keeps)
    out.append(capi.pairing_product_is_one(g1[j] + negc(g1[j + k]), g2[k] + g2[0]))
    out.append(capi.pairing_product_is_one(g1[j] + negc(g1[j + k + 1]), g2[k] + g2[0]))
    out.append(capi.pairing_product_is_one(g1[j + 1] + negc(g1[j + k]), g2[k] + g2[0]))
out.append(capi.pairing_product_is_one(g1[2] + negc(g1[3]) + g1[7] + negc(g1[9]), g2[1] + g2[0] + g2[2] + g2[0]))   # four pairs
out.append(capi.pairing_product_is_one(g1[2] + negc(g1[3]) + g1[7] + negc(g1[8]), g2[1] + g2[0] + g2[2] + g2[0]))
print("".join("1" if v else "0" for v in out))
"""


def test_host_pairing_variants_agree():
    """the fixed-Q line precomputation + sparse line products (default: two pairs on two threads; and on one; and with the host's Fp product in C
    instead of fp_x86.S), the loop that walks T itself, the generic Fp12
    squaring and the plain 1268-bit final exponentiation all give the expected verdicts on bilinearity cases over
    thirteen distinct G2 points of the tau = 1337 setup"""
    import sys
    code = _PAIRING_CASES % (ROOT, os.path.join(ROOT, "tests", "golden"), SETUP_PATH)
    want = "100" * 12 + "10"
    for var in ({}, {"LWKZG_HOST_FP_PORTABLE": "1"}, {"LWKZG_PAIRING_ONE_THREAD": "1"}, {"LWKZG_PAIRING_NO_PRECOMP": "1"}, {"LWKZG_PAIRING_GENERIC_SQR": "1"},
                {"LWKZG_PAIRING_NAIVE": "1", "LWKZG_PAIRING_NO_PRECOMP": "1"}):
        env = dict(os.environ, LWKZG_EXPERIMENTAL="1", **var)     # (cross-check arms are experiment knobs: csrc/knobs.h)
        got = subprocess.check_output([sys.executable, "-c", code], env=env).decode().strip().splitlines()[-1]
        assert got == want, (var, got)


def test_host_fiat_shamir_digests_match_hashlib(K):
    """the host-pointer proof entry points hash on the host (SHA extensions when present): same bytes as hashlib"""
    import hashlib
    import blobs as B
    from lambdaworks_kzg_amd import capi
    blobs = [B.synthetic_blob(i) for i in range(5)] + [B.make_blob("all_ff")]
    comms = [bytes([0x80 + i]) + bytes(range(47)) for i in range(len(blobs))]
    got = capi.challenge_digests_host(b"".join(blobs), b"".join(comms))
    for b, c, g in zip(blobs, comms, got):
        msg = b"FSBLOBVERIFY_V1_" + (4096).to_bytes(8, "little") + (0).to_bytes(8, "little") + b + c
        assert g == hashlib.sha256(msg).digest()


def test_batch_challenge_matches_hashlib(K):
    """r of verify_blob_kzg_proof_batch (/root/reference/src/utils.rs:166-206): the header is hashed in front of the transcript without
    building the concatenation (sha256_fast_prefixed); transcript lengths on every side of a block boundary, both byte orders"""
    import hashlib
    import random
    from lambdaworks_kzg_amd import capi
    from conftest import R
    rnd = random.Random(66)
    for n in (0, 1, 2, 3, 4, 5, 7, 64, 301):
        rec = bytes(rnd.getrandbits(8) for _ in range(160 * n))
        dg = hashlib.sha256(b"RCKZGBATCH___V1_" + (4096).to_bytes(8, "little") + n.to_bytes(8, "little") + rec).digest()
        assert capi.batch_challenge_host(rec, n, K.MODE_REFERENCE) == (int.from_bytes(dg, "big") % R).to_bytes(32, "big"), n
        assert capi.batch_challenge_host(rec, n, K.MODE_CKZG) == (int.from_bytes(dg, "little") % R).to_bytes(32, "big"), n


def test_product_arithmetic_host_crosscheck(tmp_path):
    """The kernels' own field / group sources (LWK_HD), compiled for the host: division-step inversion vs Fermat,
    28-bit-limb lazy field vs the 32-bit CIOS field, hot-loop XYZZ scalar multiplication vs the CIOS one
    (tools/host_check.hip). No GPU, no oracle: the product checked against itself along independent routes."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "host_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-I", os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"),
                           os.path.join(ROOT, "tools", "host_check.hip"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("ok:"), out


def test_direct_table_plan_constants(K):
    """window plan of the opt-in direct table: pure host arithmetic, callable without a GPU"""
    from lambdaworks_kzg_amd import capi
    l = K.lib()
    assert [l.lwkzg_direct_num_windows(b) for b in (9, 10, 11, 12, 13, 14, 15, 16, 17)] == [0, 26, 24, 22, 20, 19, 17, 16, 0]
    # 15 signed windows of 2^15 rows + one 15-bit top window of 2^15 rows, per point, 112 bytes per row
    assert capi.direct_table_bytes(16) == (15 * 4096 * 32768 + 4096 * 32768) * 112 == 240518168576
    assert capi.direct_table_bytes(15) == (16 * 4096 * 16384 + 4096 * 32768) * 112
    assert capi.direct_table_bytes(14) == (18 * 4096 * 8192 + 4096 * 8) * 112
    assert capi.direct_table_bytes(13) == (19 * 4096 * 4096 + 4096 * 256) * 112 == 35_819_356_160   # the default engine on an empty MI355X
    assert capi.direct_table_bytes(10) == (25 * 4096 * 512 + 4096 * 32) * 112
    # rows aligned to 128-byte lines (chosen when the table leaves 8 GiB of the device free): 8/7 of the packed size
    assert capi.direct_table_bytes(13, 128) == 40_936_407_040 and capi.direct_table_bytes(16, 128) == 274_877_906_944
    for bits in range(10, 17):   # every scalar bit is covered exactly once: (NW - 1) * bits + top == 255
        nw = l.lwkzg_direct_num_windows(bits)
        assert 0 < 255 - bits * (nw - 1) <= bits


def test_c_consumers_compile_and_link_against_the_header_and_library(tmp_path):
    """the C programs of tests/ (the fuzz-harness-style consumer, the lib_test.rs mirror, the multi-device consumer) build against
    include/lambdaworks_kzg_amd.h and link against the shared library with a plain C compiler; running them needs a GPU"""
    lib_dir = os.path.join(ROOT, "lambdaworks_kzg_amd", "lib")
    for src in ("c_abi_harness.c", "lib_test_mirror.c", "multi_harness.c"):
        exe = str(tmp_path / src.replace(".c", ""))
        subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", src), "-o", exe, "-L", lib_dir, "-llambdaworks_kzg",
                               "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
        assert os.path.exists(exe)


def test_one_shard_rule_from_c_and_python(tmp_path):
    """csrc/multi.hip cut its shards at floor(n k / G) while dist.py and the header said ceil -- both contiguous, two rules
    for one contract. There is ONE function now (lwkzg_shard_range: part k owns [ceil(k n / G), ceil((k + 1) n / G)), i.e. item i belongs
    to part floor(i G / n)); multi.hip uses it, dist.shard_range states the same closed form (no native library needed to compute a slice: ADVICE r05) and capi.shard_range is the binding. A C program prints it for fewer items than parts, one more
    than parts, none at all, and the bench's shapes; the closed form and the Python binding must agree line by line."""
    from lambdaworks_kzg_amd import capi, dist as D
    lib_dir = os.path.join(ROOT, "lambdaworks_kzg_amd", "lib")
    exe = str(tmp_path / "shard_rule")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shard_rule_harness.c"), "-o", exe, "-L", lib_dir, "-llambdaworks_kzg",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    cases = [(3, 8), (9, 8), (0, 8), (8, 8), (1, 1), (0, 1), (5, 2), (7, 3), (4096, 8), (1024, 3), (256, 5)]
    out = subprocess.check_output([exe] + [str(x) for c in cases for x in c], text=True).split("\n")
    rows = [tuple(int(x) for x in l.split()) for l in out if l.strip()]
    assert len(rows) == sum(g for _, g in cases)
    for n, g, k, first, count in rows:
        lo, hi = -(-k * n // g), -(-(k + 1) * n // g)
        assert (first, count) == (lo, hi - lo), (n, g, k)
        assert D.shard_range(n, g, k) == (first, count) == capi.shard_range(n, g, k)
        for i in range(first, first + count):
            assert D.owner_of(i, n, g) == k == i * g // n
    src = open(os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc", "multi.hip")).read()
    assert "n * k / parts" not in src       # the old floor rule


def test_generated_constant_tables_are_current():
    """field29_consts.inc / fr28_consts.inc are what tools/gen_field_consts.py prints (p, r, their Montgomery constants and
    the borrowed multiples the lazy subtractions add)."""
    gen = os.path.join(ROOT, "tools", "gen_field_consts.py")
    csrc = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")
    assert subprocess.check_output([sys.executable, gen]).decode() == open(os.path.join(csrc, "field29_consts.inc")).read()
    assert subprocess.check_output([sys.executable, gen, "--fr28"]).decode() == open(os.path.join(csrc, "fr28_consts.inc")).read()


def test_transform_lazy_bounds_walkthrough():
    """The 4096-point transform (fr_ops.hip: k_ntt4096) never reduces and ripples carries once: walk its twelve stages
    with the bounds fr28.cuh states -- a sum adds the limb bounds, a difference adds two units of 2^28 per limb and 4r to
    the value, a product's result is one unit per limb and < 2r -- and check what the kernel relies on: no limb passes
    the 15 units a 32-bit word holds, every product's column fits 64 bits, values stay under 2^25 r (the Montgomery
    radix 2^280 over r), and the top limb fits the 16 bits it gets in LDS."""
    n, norm_stage = 4096, 6
    r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    limb = [1] * n        # units of 2^28
    val = [2] * n         # units of r: elements enter through a product
    worst_limb = worst_val = 0
    for s in range(12):
        half = 1 << s
        nl, nv = limb[:], val[:]
        for b in range(n // 2):
            k = b & (half - 1)
            i0 = ((b >> s) << (s + 1)) + k
            i1 = i0 + half
            lu, vu = (1, val[i0]) if s == norm_stage else (limb[i0], val[i0])
            if s != 0:      # v goes through a product with a canonical twiddle
                assert 10 * (limb[i1] * 1 + 1) * (1 << 56) + (1 << 36) < 1 << 64      # column of a*b + m*r plus the carry
                assert val[i1] * 1 <= 1 << 25
                lv, vv = 1, 2
            else:
                lv, vv = limb[i1], val[i1]
                assert lv == 1 and vv == 2      # the subtraction below wants a product's result
            nl[i0], nv[i0] = lu + lv, vu + vv
            nl[i1], nv[i1] = lu + 2, vu + 4
        limb, val = nl, nv
        worst_limb, worst_val = max(worst_limb, max(limb)), max(worst_val, max(val))
    assert worst_limb == 13 and worst_limb <= 15
    assert worst_val <= 50 and worst_val * r < 1 << 280
    assert (worst_val * r) >> 252 < 1 << 16      # limb 9 as a halfword
    # the exit product takes the laziest element
    assert 10 * (worst_limb + 1) * (1 << 56) + (1 << 36) < 1 << 64


def test_every_environment_knob_is_in_the_integration_table(K):
    """the getenv knobs of csrc/ were documented in five places; VERDICT r05: 37 of them, read in the middle of functions.
    r06: ONE file reads the environment (csrc/knobs.hip, once), nothing else in the library calls getenv, the knobs come in two classes
    -- operational (always honoured; at most 20) and experiment (A/B arms, honoured only with LWKZG_EXPERIMENTAL=1) -- and INTEGRATION.md
    carries one table per class: a knob without a row (or a row without a knob) fails here."""
    src_dir = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")
    for f in os.listdir(src_dir):
        if f.endswith((".hip", ".h", ".cuh", ".inc")) and f != "knobs.hip":
            assert "getenv(" not in open(os.path.join(src_dir, f)).read(), f
    read = set(re.findall(r'"(LWKZG_[A-Z_0-9]+)"', open(os.path.join(src_dir, "knobs.hip")).read().split("knob_names_operational()")[0]))
    rep = K.knob_report()
    size = K.lib().lwkzg_knob_report(None, 0)      # the report's length with its terminator: what a caller allocates
    buf = C.create_string_buffer(size)
    assert K.lib().lwkzg_knob_report(buf, size) == size
    assert len(buf.value) == size - 1 and json.loads(buf.value.decode()) == rep
    op, ex = set(rep["operational"].split()), set(rep["experimental_names"].split())
    assert not (op & ex) and op | ex == read, (sorted(read - (op | ex)), sorted((op | ex) - read))
    assert len(op) <= 20, len(op)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    op_doc, ex_doc = doc.split("<!-- experiment knobs -->")
    rows_op = set(re.findall(r"^\s*\| `(LWKZG_[A-Z_0-9]+)` \|", op_doc, flags=re.M))
    rows_ex = set(re.findall(r"^\s*\| `(LWKZG_[A-Z_0-9]+)` \|", ex_doc, flags=re.M))
    assert rows_op == op, (sorted(op - rows_op), sorted(rows_op - op))
    assert rows_ex == ex, (sorted(ex - rows_ex), sorted(rows_ex - ex))


def test_glv_split_by_barrett_equals_the_restoring_division(tmp_path):
    """csrc/glv.cuh as plain C++: k = lo + hi z^2 by Barrett's reduction (k_vmsm_scalars, behind r on the verification's critical path)
    against the bitwise restoring division (k_lincomb3, the r05 arm) on edge values and 10^6 random integers below 2^255"""
    exe = str(tmp_path / "glv_split_check")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "glv_split_check.cpp"), "-o", exe])
    n, bad = (int(x) for x in subprocess.check_output([exe], text=True).split())
    assert n > 1000000 and bad == 0


def test_host_scalar_products_of_a_verification(K, oracle, oracle_setup):
    """verify_kzg_proof (/root/reference/src/lib.rs:407-456) is host arithmetic end to end, so it runs here on a KZGSettings put together by hand
    (the oracle's points in the blst layout, no context): [y]G over the generator's window table and [z]pi over the endomorphism
    split (verify.hip: generator_mul, scalar_mul) against the oracle's own products, on scalars around every boundary of the two --
    nibble carries, the 128-bit halves, multiples of z^2, r - 1 -- with C = [y + (tau - z) a]G, pi = [a]G, tau = 1337."""
    import ctypes as C
    import random
    import struct
    from conftest import R
    from lambdaworks_kzg_amd import capi

    def blst_fp(be48):
        return struct.pack("<6Q", *[int.from_bytes(be48[8 * k:8 * k + 8], "big") for k in range(6)])

    g2 = b""
    for k in (1, 1337):
        xy = oracle.g2_generator_mul(k)
        g2 += b"".join(blst_fp(xy[48 * j:48 * j + 48]) for j in range(4)) + blst_fp((1).to_bytes(48, "big")) + blst_fp(bytes(48))
    g1 = oracle_setup.g1_blst()[:144]
    g1_buf, g2_buf = C.create_string_buffer(g1, len(g1)), C.create_string_buffer(g2, len(g2))
    s = capi.KZGSettings()
    s.fs, s.g1_values, s.g2_values = None, C.addressof(g1_buf), C.addressof(g2_buf)
    zsq = 0xac45a4010001a4020000000100000000
    rnd = random.Random(77)
    edge = [0, 1, 2, 15, 16, 17, 2 ** 64, 2 ** 128 - 1, 2 ** 128, 2 ** 128 + 1, zsq - 1, zsq, zsq + 1, 5 * zsq, (2 ** 127) * 2 + zsq,
            R - 1, R - 2, R - zsq, (R - 1) // 2, int("f" * 63, 16) % R, int("8" * 64, 16) % R]
    cases = [(y, z) for y in edge for z in (3, R - 1)] + [(7, z) for z in edge] + [(rnd.randrange(R), rnd.randrange(R)) for _ in range(24)]
    ok = C.c_bool(False)
    for i, (y, z) in enumerate(cases):
        a = rnd.randrange(1, R) if i % 5 else 0            # a = 0: the proof is the point at infinity
        cm = oracle.g1_generator_mul((y + (1337 - z) * a) % R)
        pi = oracle.g1_generator_mul(a)
        zb, yb = z.to_bytes(32, "big"), y.to_bytes(32, "big")
        assert capi.lib().verify_kzg_proof(C.byref(ok), cm, zb, yb, pi, C.byref(s)) == 0 and ok.value is True, (i, hex(y), hex(z))
        yb2 = ((y + 1) % R).to_bytes(32, "big")
        assert capi.lib().verify_kzg_proof(C.byref(ok), cm, zb, yb2, pi, C.byref(s)) == 0 and ok.value is False, (i, hex(y), hex(z))
        if a:
            zb2 = ((z + 1) % R).to_bytes(32, "big")
            assert capi.lib().verify_kzg_proof(C.byref(ok), cm, zb2, yb, pi, C.byref(s)) == 0 and ok.value is False, (i, hex(y), hex(z))


def test_host_decompression_of_a_verification(K, oracle, oracle_setup):
    """decompress_g1_point (/root/reference/src/compression.rs:62-103) as verify_kzg_proof runs it on the host (verify.hip: host_decompress_nocheck --
    the square root on 64-bit limbs -- then the endomorphism subgroup test): accept / reject equals the oracle's on valid points under
    both sign bits, infinity encodings with stray bits, missing flags, x off the curve, x on the curve outside G1, x >= p; and an accepted
    encoding decodes to the oracle's point (the sign of y: C = +-[k]G verifies against y = +-k with the proof at infinity)."""
    import ctypes as C
    import random
    import struct
    from conftest import R
    from lambdaworks_kzg_amd import capi
    P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab

    def blst_fp(be48):
        return struct.pack("<6Q", *[int.from_bytes(be48[8 * k:8 * k + 8], "big") for k in range(6)])

    g2 = b""
    for k in (1, 1337):
        xy = oracle.g2_generator_mul(k)
        g2 += b"".join(blst_fp(xy[48 * j:48 * j + 48]) for j in range(4)) + blst_fp((1).to_bytes(48, "big")) + blst_fp(bytes(48))
    g1 = oracle_setup.g1_blst()[:144]
    g1_buf, g2_buf = C.create_string_buffer(g1, len(g1)), C.create_string_buffer(g2, len(g2))
    s = capi.KZGSettings()
    s.fs, s.g1_values, s.g2_values = None, C.addressof(g1_buf), C.addressof(g2_buf)
    inf = bytes([0xc0]) + bytes(47)
    rnd = random.Random(99)
    ok = C.c_bool(False)

    def lib_verdict(c48, y):
        rc = capi.lib().verify_kzg_proof(C.byref(ok), c48, bytes(32), (y % R).to_bytes(32, "big"), inf, C.byref(s))
        return None if rc != 0 else bool(ok.value)

    # valid points: both sign bits decode to the oracle's point and its negative
    for i in range(40):
        k = rnd.randrange(1, R)
        c = oracle.g1_generator_mul(k)
        flipped = bytes([c[0] ^ 0x20]) + c[1:]
        assert lib_verdict(c, k) is True and lib_verdict(c, R - k) is False
        assert lib_verdict(flipped, R - k) is True and lib_verdict(flipped, k) is False
        assert oracle.g1_compress(*oracle.g1_decompress(flipped)) == oracle.g1_generator_mul(R - k)
    # accept / reject on everything else
    cands = [inf, bytes([0xc0]) + bytes([0xff] * 47), bytes([0xe0 | 0x1f]) + bytes(range(47)), bytes([0x40]) + bytes(47), bytes(48), bytes([0x20]) + bytes(47),
             bytes([0x80]) + bytes(47), bytes([0xa0]) + bytes(47)]                       # x = 0: (0, +-2) is on the curve, of order 3
    good = oracle.g1_generator_mul(12345)
    cands += [bytes([good[0] & 0x7f]) + good[1:], bytes([good[0] | 0x40]) + good[1:]]    # compression flag cleared; infinity flag set on a point
    for _ in range(300):
        x = rnd.randrange(P)
        cands.append(bytes([0x80 | (0x20 if rnd.random() < 0.5 else 0)]) + bytes(47))   # replaced below
        b = bytearray(x.to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if rnd.random() < 0.5 else 0)
        cands[-1] = bytes(b)
    xg = int.from_bytes(bytes([good[0] & 0x1f]) + good[1:], "big")
    for x in (xg + P, P, P + 1, (1 << 381) - 1):                                         # x >= p inside 381 bits
        if x < (1 << 381):
            b = bytearray(x.to_bytes(48, "big"))
            b[0] |= 0x80 | (good[0] & 0x20)
            cands.append(bytes(b))
    n_acc = 0
    for c in cands:
        want = oracle.g1_decompress(c)
        got = lib_verdict(c, 0)
        if want is None:
            assert got is None, c.hex()
        else:
            n_acc += 1
            assert got is want[1], c.hex()      # e(C, G2) == 1 exactly when C is the point at infinity
    assert n_acc >= 3
