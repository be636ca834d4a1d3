"""GPU: the DEVICE build of the primitives (tests/prims_check.hip, one case per lane, one kernel per family) held to Python integers
(tests/prims_cases.py) on operands at the bounds their types declare. What only the device compile has: operator* and sqr as calls of
mont_mul29_call / mont_sqr29_call or as inlined bodies, mul_sub<INL = true> as ONE fused mont_mul_add29 over neg(c), fe_mul as
fe_mul_call, and the G1Xyzz29i / G1Affine29i instantiations of the group law. The host compile of the same cases is
tests/test_prims_cpu.py."""
import pytest

import prims_cases
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_run(tmp_path_factory):
    exe, build_seconds = prims_cases.build_checker(ROOT, str(tmp_path_factory.mktemp("prims_dev")), host_only=False)
    assert exe is not None, "hipcc is needed to build tests/prims_check.hip"
    # one process, one launch set: process start, six kernels of a few thousand lanes, well under a second of GPU work
    cases, results, run_seconds = prims_cases.run_checker(exe, "device", str(tmp_path_factory.mktemp("prims_dev_io")), timeout=120)
    print("prims_check: built in %.1f s, device run %.2f s, %d cases" % (build_seconds, run_seconds, len(cases)))
    return cases, results


@pytest.mark.parametrize("family", prims_cases.FAMILIES)
def test_device_build_agrees_with_big_integers(device_run, family):
    """the comparisons of tests/test_prims_cpu.py, on what the kernels computed; the inlined mul_sub must declare < 2p here (the fused
    branch) and stay below it"""
    cases, results = device_run
    prims_cases.check_family(family, cases, results)
