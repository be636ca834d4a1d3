"""CPU: the padded launch of lambdaworks_kzg_amd/csrc/lds_pad.h (the LDS footprint that keeps the validation kernels off the hash's
compute units: k_validate_commitments, k_decompress_points, k_subgroup_coop_asm, k_vmsm_multiples, k_point_multiples) compiled for the
host under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, tests/lds_pad_check.cpp, against a fake runtime
that records the dynamic LDS of every launch and can refuse: the pads of the default knobs pass unchanged (56 + 60 KiB and 116 KiB under
the 160 KiB of a gfx950 workgroup), a pad that does not fit is cut to limit - static, a refused pad is launched again without one and
latched for that kernel on that device only, and a pending error is neither cleared nor mistaken for a refusal."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")
KIB = 1024

# name: the launches' dynamic LDS | the error pending afterwards | the (kernel, device) latch | LDS queries made
WANT = [
    ("fit 56+60", [60 * KIB], 0, 0, 2),
    ("fit 56+60 again", [60 * KIB], 0, 0, 0),
    ("fit 0+116", [116 * KIB], 0, 0, 2),
    ("no pad wanted", [0], 0, 0, 0),
    ("clamp 56+150", [160 * KIB - 56 * KIB], 0, 0, 2),
    ("clamp 0+150", [150 * KIB], 0, 0, 2),
    ("static above limit", [0], 0, 0, 2),
    ("refused first", [116 * KIB, 0], 0, 1, 2),
    ("refused later", [0], 0, 1, 0),
    ("other device", [116 * KIB], 0, 0, 2),
    ("other kernel", [116 * KIB], 0, 0, 2),
    ("ordinal beyond the table", [0], 0, 0, 0),
    ("both refused", [116 * KIB, 0], 98, 1, 2),
    ("pending", [0], 719, 0, 0),
    ("attribute refused", [0], 0, 1, 2),
]


def test_padded_launch_clamps_falls_back_and_latches_per_kernel_and_device(tmp_path):
    assert 60 * KIB == 61440 and 116 * KIB == 118784 and 160 * KIB - 56 * KIB == 106496 and 150 * KIB == 153600
    exe = str(tmp_path / "lds_pad_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "lds_pad_check.cpp")])
    run = subprocess.run([exe], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    lines = out.strip().split("\n")
    want = ["%s: %s | pending %d | refused %d | queries %d" % (name, ",".join(str(v) for v in calls), pending, refused, queries)
            for name, calls, pending, refused, queries in WANT]
    assert lines == want, out
