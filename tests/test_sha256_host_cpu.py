"""CPU: the host SHA-256 of lambdaworks_kzg_amd/csrc/sha256_host.hip -- the portable compression (sha256_host, which a host with the SHA
extensions otherwise never compares with anything), the routine that takes the extensions when present (sha256_fast) and the one that
hashes prefix | message without the concatenation -- against hashlib, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/sha256_host_check.cpp). Lengths on every side of the padding's boundaries (55 | 56, 63 | 64 | 65,
119 | 120, 127 | 128), the empty message with null pointers, and a few thousand bytes."""
import hashlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")
LENS = [0, 1, 31, 32, 33, 55, 56, 57, 62, 63, 64, 65, 119, 120, 127, 128, 129, 191, 192, 1000, 4096]


def test_host_sha256_portable_fast_and_prefixed_match_hashlib(tmp_path):
    exe = str(tmp_path / "sha256_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-x", "c++",
                           "-I", CSRC, os.path.join(ROOT, "tests", "sha256_host_check.cpp"), "-o", exe, "-lpthread"])
    run = subprocess.run([exe] + [str(n) for n in LENS], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    msg = bytes((i * 7 + 3) & 255 for i in range(4096))
    seen = {"host": 0, "fast": 0, "prefixed": 0}
    for line in out.strip().split("\n"):
        n, name, hexd = line.split()
        assert hexd == hashlib.sha256(msg[:int(n)]).hexdigest(), line
        seen[name] += 1
    assert seen["host"] == len(LENS) and seen["fast"] == len(LENS) and seen["prefixed"] >= 3 * len(LENS), seen
