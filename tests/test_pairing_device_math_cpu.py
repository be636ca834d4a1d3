"""The per-item verification's pairing (lambdaworks_kzg_amd/csrc/fp12.cuh) compiled for the HOST and checked without a GPU
(tools/pairing_dev_check.hip): tower identities, the line tables the library uploads against an independent affine walk, and the
verdict of e(P, G2) e(-pi, [tau]G2) == 1 against the host pairing of the library (lwkzg_pairing_product_is_one)."""
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT, SETUP_PATH, TAU, R, P


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("pdc") / "pairing_dev_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--cuda-host-only", "-I", os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc"),
                           os.path.join(ROOT, "tools", "pairing_dev_check.hip"), "-o", exe])
    tmp = tmp_path_factory.mktemp("pdc_in")

    def run(lines):
        path = str(tmp / "cmds.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        return subprocess.check_output([exe, path], timeout=600).decode().split("\n")[:-1]
    return run


def _coords(xy192):
    return [xy192[48 * k:48 * (k + 1)].hex() for k in range(4)]


@pytest.fixture(scope="module")
def g2_points(oracle, oracle_setup):
    g2, tg2 = oracle.g2_generator_mul(1), oracle.g2_generator_mul(TAU)
    # the tau = 1337 setup's g2_values[0] and [1] are exactly these points
    assert oracle_setup.g2_compressed()[:192] == oracle.g2_compress(g2) + oracle.g2_compress(tg2)
    return g2, tg2


def test_tower_identities(checker):
    """a a^-1 = 1; cyclotomic square = generic square = product on cyclotomic elements; frob_p^12 = id, frob_p^2 = frob_p2; exp_by_x"""
    assert checker(["selftest 24"]) == ["selftest ok"]


def test_line_tables_equal_fixed_q_lines(K, oracle, checker, g2_points):
    """what the library uploads per context (pairing.hip: fixed_q_lines, converted) == an independent affine walk on the device tower,
    for G2 and [tau]G2 of the tau = 1337 setup"""
    from lambdaworks_kzg_amd import capi
    for q in g2_points:
        lib_table = capi.pairing_line_table(oracle.g2_compress(q))
        assert len(lib_table) == 68 * 192
        (walk,) = checker(["lines " + " ".join(_coords(q))])
        assert walk == lib_table.hex()


def _neg_compressed(c48):
    if c48[0] & 0x40:  # infinity
        return c48
    return bytes([c48[0] ^ 0x20]) + c48[1:]


def test_device_verdicts_match_host_pairing(K, oracle, checker, g2_points):
    """e(P, G2) e(-pi, [tau]G2) == 1 by the device code == lwkzg_pairing_product_is_one: matching pairs (P = [tau]pi), non-matching
    ones, and points at infinity on either side"""
    from lambdaworks_kzg_amd import capi
    rnd = random.Random(4242)
    inf = bytes([0xc0]) + bytes(47)
    cases = []
    for i in range(240):
        k = rnd.randrange(1, R)
        pi = oracle.g1_generator_mul(k)
        kind = i % 6
        if kind in (0, 1, 2):
            p = oracle.g1_generator_mul(TAU * k % R)                       # matching
        elif kind == 3:
            p = oracle.g1_generator_mul((TAU * k + rnd.randrange(1, R)) % R)   # not matching
        elif kind == 4:
            p = oracle.g1_generator_mul(TAU * k % R)
            pi = oracle.g1_generator_mul(k + 1)                            # pi off by one
        else:
            p = oracle.g1_generator_mul(rnd.randrange(1, R))
        cases.append((p, pi))
    k = rnd.randrange(1, R)
    cases += [(inf, inf), (inf, oracle.g1_generator_mul(k)), (oracle.g1_generator_mul(k), inf),
              (oracle.g1_generator_mul(0), oracle.g1_generator_mul(R))]   # [0]G and [r]G: infinity as the oracle encodes it
    g2, tg2 = g2_points
    cmds = ["q 0 " + " ".join(_coords(g2)), "q 1 " + " ".join(_coords(tg2))]
    cmds += ["pair %s %s" % (p.hex(), pi.hex()) for p, pi in cases]
    got = checker(cmds)
    assert len(got) == len(cases)
    g2c = oracle.g2_compress(g2) + oracle.g2_compress(tg2)
    n_true = 0
    for (p, pi), dev in zip(cases, got):
        want = capi.pairing_product_is_one(p + _neg_compressed(pi), g2c)
        assert dev == str(int(want)), (p.hex(), pi.hex())
        n_true += want
    assert 100 < n_true < len(cases) - 60   # both outcomes well represented
