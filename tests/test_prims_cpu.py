"""The primitives beneath every kernel -- the lazy field F29<B, INL, LB> (field29.cuh), the XYZZ group law on it (g1.cuh), fr28.cuh, the
CIOS Fp / Fr and the GLV split -- compiled for the HOST (tests/prims_check.hip) and held to Python integers (tests/prims_cases.py) on
operands that sit AT the bounds the types declare: saturated lazy limbs, values one below B p, every multiple of p a type admits. The
device compile of the same cases is tests/test_gpu_prims.py."""
import pytest

import prims_cases
from conftest import ROOT


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    exe, _ = prims_cases.build_checker(ROOT, str(tmp_path_factory.mktemp("prims_host")), host_only=True)
    if exe is None:
        pytest.skip("hipcc not available")
    cases, results, _ = prims_cases.run_checker(exe, "host", str(tmp_path_factory.mktemp("prims_host_io")), timeout=120)
    return cases, results


@pytest.mark.parametrize("family", prims_cases.FAMILIES)
def test_host_build_agrees_with_big_integers(host_run, family):
    """A products: = a b 2^-392 (a b - c d for mul_sub) mod p, < (declared bound) p, limbs 0..12 < (declared LIMB) 2^28;
    B sums and tests: the same, is_zero on every k p a type admits and on k p +- 1, is_literal_zero; neg / cneg(., true) of the literal
    zero give exactly K p (<=), everything else is < its bound;  C conversions, inversions, the square-root power;
    D the group law against a pure-Python affine law, accumulators with X up to 13 p, Y up to 5 p, ZZ / ZZZ up to p above the residue;
    E fr28 at its header's bounds, the CIOS fields, both splits against divmod(k, z^2)"""
    cases, results = host_run
    prims_cases.check_family(family, cases, results)


def test_the_case_lines_satisfy_their_slots():
    """the generators themselves: a saturated operand is the largest below B p with limbs LB 2^28 - 1, a lazy decomposition keeps the
    integer and the limb bound"""
    import random
    rnd = random.Random(29)
    for b, lb in [(1, 1), (2, 1), (14, 5), (31, 7), (1, 14), (2048, 1), (1024, 4)]:
        s = prims_cases.saturated(b, lb)
        assert prims_cases.val(s) < b * prims_cases.P <= prims_cases.val(s) + (1 << 364)
        assert all(l == (lb << 28) - 1 for l in s[:13])
        v = rnd.randrange(b * prims_cases.P)
        l = prims_cases.lazy(v, lb, rnd)
        assert prims_cases.val(l) == v and all(x < lb << 28 for x in l[:13])
    assert len(prims_cases.build_cases("host")) == len(prims_cases.build_cases("device"))
