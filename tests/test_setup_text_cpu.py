"""CPU: the host-only parser of the two c-kzg-4844 trusted setup texts (lambdaworks_kzg_amd/csrc/setup_text.h) as a stand-alone program,
tests/setup_text_check.cpp, under AddressSanitizer and UndefinedBehaviorSanitizer: both layouts; LF, CRLF, tabs and runs of blanks; a
trailing newline and none; a text cut in the middle of a token; an empty file; counts of 20 digits; tokens that are not hex or of the
wrong length. This covers the parser alone: nothing that is loaded into python runs under a sanitizer here."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "lambdaworks_kzg_amd", "csrc")


def test_setup_text_parser_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "setup_text_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "setup_text_check.cpp")])
    run = subprocess.run([exe], capture_output=True)
    out = run.stdout.decode()
    assert run.returncode == 0, out + run.stderr.decode()
    assert "setup_text ok" in out and "FAILED" not in out
