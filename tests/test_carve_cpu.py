"""CPU: the carver of lambdaworks_kzg_amd/csrc/carve.h (one allocation cut into 256-byte aligned pieces: the cell verifiers' buffers
and the batch verification's vmsm scratch) compiled for the host under AddressSanitizer and UndefinedBehaviorSanitizer as a
stand-alone program, tests/carve_check.cpp. For capacities on both sides of the buffers' first sizes (64, 256) and a piece list with
sizes 0, 1, 255, 256 and 257 in it: every pointer is 256-aligned, the pieces neither overlap nor leave the block, and the probe from
a null base reports the total the real carve uses."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")
CAPS = [1, 63, 64, 65, 256, 257]


def test_carver_pieces_are_aligned_disjoint_and_probed_alike(tmp_path):
    exe = str(tmp_path / "carve_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "carve_check.cpp")])
    run = subprocess.run([exe] + [str(c) for c in CAPS], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    lines = out.strip().split("\n")
    assert len(lines) == len(CAPS) and all(line.endswith(" ok") for line in lines), out
    for cap, line in zip(CAPS, lines):
        # sizes 0 | 1 | 4 cap | 8 cap + 8 | 255 | 256 | 257 | 33 cap, each rounded up to 256
        want = sum((b + 255) // 256 * 256 for b in (0, 1, 4 * cap, 8 * cap + 8, 255, 256, 257, 33 * cap))
        assert line == "cap %d: %d bytes ok" % (cap, want), line
