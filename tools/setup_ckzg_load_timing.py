"""Where the milliseconds of a c-kzg-4844 trusted setup load go, beside the parent's way to the same state.

    python tools/setup_ckzg_load_timing.py [OUT]      # OUT defaults to profiles/setup_ckzg_load_timing.txt

Four loads per form in ONE process (the first pays the runtime's start), wall-clock milliseconds and the stages of lwkzg_timing_report:
  * one-section   lwkzg_load_trusted_setup_file_ckzg on the text of tests/golden/make_lagrange_setup.py (c-kzg 1.x: the monomial points are derived)
  * three-section lwkzg_load_trusted_setup_ckzg on the same setup's three sections (c-kzg 2.x: nothing derived, the sections cross-checked)
  * parent        load_trusted_setup_file on tests/golden/trusted_setup.txt followed by lwkzg_settings_set_mode(CKZG): the only way to
                  a c-kzg-mode settings object with both forms before these loaders existed (the Lagrange form derived from the monomial)
Every form ends with both forms of the setup live and the default engine's table(s) built. Not yet timed on an MI355X: DESIGN.md
section 4l says what is expected until profiles/setup_ckzg_load_timing.txt exists."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import lambdaworks_kzg_amd as K  # noqa: E402
from lambdaworks_kzg_amd import capi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLDEN, "trusted_setup.txt")


def sections(path):
    with open(path) as f:
        t = f.read().split()
    return b"".join(bytes.fromhex(x) for x in t[2:2 + 4096]), b"".join(bytes.fromhex(x) for x in t[2 + 4096:])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "setup_ckzg_load_timing.txt")
    import tempfile
    import make_lagrange_setup as L
    LAG = L.write(tempfile.mkdtemp())   # the c-kzg 1.x text of the same setup (pinned by digest; about 4 s on the CPU)
    mono, g2 = sections(MONO)
    lag, _ = sections(LAG)
    lines = ["# tools/setup_ckzg_load_timing.py: four loads per form in one process; wall-clock ms of the host thread", "# " + K.lib().lwkzg_version().decode()]
    capi.runtime_init()

    def parent():
        ts = K.TrustedSetup.from_file(MONO)
        t = time.perf_counter()
        ts.set_mode(K.MODE_CKZG)
        ts.set_mode_ms = (time.perf_counter() - t) * 1e3
        return ts

    forms = (("one-section (file, c-kzg 1.x)", lambda: K.TrustedSetup.from_ckzg_file(LAG)),
             ("three-section (bytes, c-kzg 2.x)", lambda: K.TrustedSetup.from_ckzg_bytes(mono, lag, g2)),
             ("parent: load_trusted_setup_file + lwkzg_settings_set_mode(CKZG)", parent))
    for name, load in forms:
        for k in range(4):
            t = time.perf_counter()
            ts = load()
            ms = (time.perf_counter() - t) * 1e3
            rep = ts.timing_report()
            extra = " (of which set_mode %.1f)" % ts.set_mode_ms if hasattr(ts, "set_mode_ms") else ""
            lines.append("%s  run %d: %.1f ms%s  bits %d forms %d  load stages %s" % (name, k, ms, extra, ts.direct_table_bits(), ts.direct_table_forms(),
                                                                                   json.dumps(rep["load"], sort_keys=True)))
            assert ts.get_mode() == K.MODE_CKZG
            ts.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
