#!/usr/bin/env python3
"""The tau = 1337 testing setup in the layout of a c-kzg-4844 1.x trusted_setup.txt: G1 in LAGRANGE form, natural order.

    python tests/golden/make_lagrange_setup.py [DIR]      # writes DIR/trusted_setup_lagrange.txt (about 5 s; default: the current directory)
    python tests/golden/make_lagrange_setup.py --check    # regenerates and compares with the pinned size and SHA-256

The text itself is not committed: it is 409,864 bytes of hex that this file regenerates in seconds, and its size and digest are pinned
below, so every user of it (the tests through write(), tools/setup_ckzg_load_timing.py) gets the same bytes or an assertion.

* trusted_setup_lagrange.txt -- "4096", "65", then 4096 compressed G1 points [l_i(tau)]G with l_i the Lagrange polynomial of the domain
  point w^i (w = 7^((r-1)/4096), the 4096th root of unity c-kzg-4844 and this library use), i = 0 .. 4095 in NATURAL order (c-kzg
  permutes them by bit reversal when it loads), then the 65 G2 lines of trusted_setup.txt unchanged. 409,864 bytes, as trusted_setup.txt.
  It is the input of the c-kzg loaders (lwkzg_load_trusted_setup_lagrange, lwkzg_load_trusted_setup_file_ckzg), and together
  with trusted_setup.txt the tests assemble the three-section (c-kzg 2.x) text from it.

      l_i(tau) = (tau^4096 - 1) / 4096 * w^i / (tau - w^i)

The scalars are plain integer arithmetic; the points come from the CPU oracle (oracle.g1_generator_mul). The tests compute the Lagrange
bytes of the other two setups (make_setups.py: tau', unstructured) with the same functions. Nothing here is product code and nothing is
read from /root/reference.
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N1, N2 = 4096, 65
TAU = 1337
OMEGA = pow(7, (R - 1) // N1, R)
FILE = "trusted_setup_lagrange.txt"
# the text is pinned, not committed: 409,864 bytes of hex for what the 40 lines below regenerate in seconds
SIZE = 409864
SHA256 = "bd7d86ec05429b663da1e25107a2ce3bc7ef1e396104bd2f50dc0c176770cc3f"


def lagrange_scalars(tau):
    """l_i(tau), i = 0 .. 4095, natural order, for a tau that is no domain point"""
    tau %= R
    head = (pow(tau, N1, R) - 1) * pow(N1, R - 2, R) % R
    out, w = [], 1
    for _ in range(N1):
        out.append(head * w % R * pow((tau - w) % R, R - 2, R) % R)
        w = w * OMEGA % R
    return out


def lagrange_scalars_of(monomial_scalars):
    """The Lagrange-form scalars of ANY 4096 scalars k_j standing where tau^j would: (1 / 4096) sum_j w^(-i j) k_j, natural order
    (an inverse DFT, radix 2, decimation in time)."""
    a = [x % R for x in monomial_scalars]
    assert len(a) == N1
    a = [a[int(format(i, "012b")[::-1], 2)] for i in range(N1)]
    winv = pow(OMEGA, R - 2, R)
    size = 2
    while size <= N1:
        step = pow(winv, N1 // size, R)
        half = size // 2
        for start in range(0, N1, size):
            t = 1
            for k in range(half):
                u, v = a[start + k], a[start + k + half] * t % R
                a[start + k], a[start + k + half] = (u + v) % R, (u - v) % R
                t = t * step % R
        size *= 2
    ninv = pow(N1, R - 2, R)
    return [x * ninv % R for x in a]


def g1_points(scalars, indices=None):
    """compressed [s]G for the scalars (all of them, or those at `indices`)"""
    from oracle import oracle as O
    O.build()
    return [O.g1_generator_mul(scalars[i]) for i in (range(len(scalars)) if indices is None else indices)]


def g2_lines():
    with open(os.path.join(HERE, "trusted_setup.txt")) as f:
        tokens = f.read().split()
    assert tokens[:2] == [str(N1), str(N2)] and len(tokens) == 2 + N1 + N2
    return tokens[2 + N1:]


def setup_text(g1, g2_hex):
    """one token per line; like trusted_setup.txt, whose last line has no newline behind it"""
    return "\n".join([str(N1), str(N2)] + [x.hex() for x in g1] + list(g2_hex))


def write(directory):
    """The text, generated (about 4 s), checked against its pinned size and digest and written to `directory`; returns the path."""
    text = setup_text(g1_points(lagrange_scalars(TAU)), g2_lines())
    assert len(text) == SIZE and hashlib.sha256(text.encode()).hexdigest() == SHA256, "the generator no longer gives the pinned text"
    path = os.path.join(directory, FILE)
    with open(path, "w") as f:
        f.write(text)
    return path


def main():
    if "--check" in sys.argv:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            write(d)
        print("the generator gives the pinned Lagrange setup")
        return
    print("wrote", write(sys.argv[1] if len(sys.argv) > 1 else os.getcwd()))


if __name__ == "__main__":
    main()
