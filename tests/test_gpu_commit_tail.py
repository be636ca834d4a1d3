"""GPU: the commitment step on one workgroup per blob (n >= 512 on the direct table) as parse, accumulate, second pass and ONE tail
launch (direct.hip: k_commit_tail -- fold, inversion and compression; the status words and the redo flags cleared by the parse kernel on
its way) against the launch set it replaces (LWKZG_COMMIT_TAIL=0: two fill launches, parse, accumulate, fold, second pass, finalize), in
fresh processes. Both arms compute the same group elements and compress them: every byte must agree, and a sample is held against
the CPU oracle and the closed forms. tests/commit_tail_worker.py is what each process runs."""
import functools
import json
import os
import subprocess
import sys

import pytest

import blobs as B
from conftest import R, ROOT, tau_closed_form

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run_arm(arm):
    """the worker's report on one arm; run once per session (tests/test_gpu_full_chunk_flags.py reads the same two reports)"""
    e = dict(os.environ, LWKZG_EXPERIMENTAL="1", LWKZG_COMMIT_TAIL=str(arm))
    e.pop("LWKZG_DIRECT_BITS", None)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tests", "commit_tail_worker.py")], env=e).decode()
    return json.loads(out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def arms():
    return {arm: run_arm(arm) for arm in (0, 1)}


def _without_profiles(r):
    return {k: ({kk: vv for kk, vv in v.items() if kk != "profile"} if isinstance(v, dict) else v)
            for k, v in r.items() if k not in ("knob", "profile_1024")}


def _split(hexstr):
    raw = bytes.fromhex(hexstr)
    return [raw[i:i + 48] for i in range(0, len(raw), 48)]


def test_arms_agree_byte_for_byte(arms):
    """commitments at 512 / 513 / 1024 / 1500 blobs on the default and a wider table, the c-kzg commitments on the Lagrange form, the
    adversarial batches and the proofs of 1024 blobs: the same bytes whichever launch set computed them; no status word left set"""
    assert arms[0]["knob"] == 0 and arms[1]["knob"] == 1
    assert arms[0]["bits"] == arms[1]["bits"] and arms[1]["bits"] >= 10
    a, b = _without_profiles(arms[0]), _without_profiles(arms[1])
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k] == b[k], k
    for k, v in b.items():
        if isinstance(v, dict):
            assert v["status_sum"] == 0, k


@pytest.mark.parametrize("n", [512, 513, 1024, 1500])
def test_reference_mode_commitments_match_the_closed_form(arms, oracle, n):
    data = B.synthetic_batch(52000 + n, n)
    tables = ("default", "wide") if n in (512, 1024) else ("default",)
    for table in tables:
        got = _split(arms[1]["%s_%d" % (table, n)]["commitments"])
        assert len(got) == n
        for i in sorted(set(list(range(0, n, 61)) + [n - 1])):
            blob = data[i * B.BYTES_PER_BLOB:(i + 1) * B.BYTES_PER_BLOB]
            assert got[i] == tau_closed_form(oracle, B.blob_scalars(blob)), (table, i)


def test_reference_mode_sample_against_the_oracle(arms, oracle, oracle_setup):
    n = 512
    data = B.synthetic_batch(52000 + n, n)
    got = _split(arms[1]["default_512"]["commitments"])
    for i in (0, 255, 511):
        assert (0, got[i]) == oracle.blob_to_kzg_commitment(data[i * B.BYTES_PER_BLOB:(i + 1) * B.BYTES_PER_BLOB], oracle_setup, oracle.MODE_R), i


def test_ckzg_mode_on_the_lagrange_form_against_the_oracle(arms, oracle, oracle_setup):
    n = 512
    got = _split(arms[1]["ckzg_lagrange_512"]["commitments"])
    assert len(got) == n
    for i in (0, 300, 511):
        assert (0, got[i]) == oracle.blob_to_kzg_commitment(B.synthetic_blob(53000 + i, big_endian=False), oracle_setup, oracle.MODE_C), i


def test_pairs_that_meet_in_the_fold_are_repaired_in_the_tail(arms, oracle):
    """equal and opposite lane sums raise the flag in the fold, behind the second pass: the tail wave folds that blob again with the
    complete addition. Every commitment against the closed form, and the profiles of the two arms show which launch did the repair."""
    from flag_cases import fold_collision_scalars
    got = _split(arms[1]["fold_collisions_512"]["commitments"])
    assert len(got) == 512
    bad = [b for b in range(512) if got[b] != tau_closed_form(oracle, fold_collision_scalars(b))]
    assert not bad, (len(bad), bad[:8])
    # WHERE the repair ran, by the library's own kernel clock. In the old launch set the second pass follows the fold: real work there
    # (512 recomputed blobs: milliseconds) says that these inputs raise their flags, and only the fold can have raised them, because ...
    old, new = arms[0]["fold_collisions_512"]["profile"], arms[1]["fold_collisions_512"]["profile"]
    assert old["k_direct_redo"]["total_ms"] > 0.2, old
    # ... the new launch set's second pass, which runs in FRONT of the fold and sees the accumulation's flags alone, found none
    # (it reads 512 flags: microseconds). The right bytes above therefore came from the tail's own repair branch.
    assert new["k_direct_redo"]["total_ms"] < 0.1, new
    assert "k_direct_fold_lanes" not in new and "k_finalize_compress" not in new and new["k_commit_tail"]["launches"] == 1, new


def test_adversarial_scalars_take_the_second_pass_and_the_next_call_starts_clean(arms, oracle):
    """the scalar sets of tests/test_gpu_setups_unstructured.py on the all-generator setup at 512 blobs: closed forms, the second pass
    doing real work under its profile name; then an honest batch on the same settings: right results, status words zero although they
    started as garbage, and a second pass that finds no flag (the clears that ride on the parse kernel are not lost)"""
    from commit_tail_worker import ADVERSARIAL
    n = 512
    r = arms[1]["adversarial_512"]
    got = _split(r["commitments"])
    for i in range(n):
        assert got[i] == oracle.g1_generator_mul(sum(ADVERSARIAL[i % len(ADVERSARIAL)]) % R), i
    assert _split(arms[1]["adversarial_512_host_pointers"]) == got
    assert r["profile"]["k_direct_redo"]["launches"] == 1
    assert r["profile"]["k_direct_redo"]["total_ms"] > 0.2, r["profile"]["k_direct_redo"]
    h = arms[1]["honest_after_adversarial_512"]
    got = _split(h["commitments"])
    for b in range(n):
        assert got[b] == oracle.g1_generator_mul(b + 2), b
    assert h["status_sum"] == 0
    # the flagged call's second pass recomputed 448 blobs (milliseconds); one that only reads 512 flags takes microseconds
    assert h["profile"]["k_direct_redo"]["total_ms"] < 0.1 < r["profile"]["k_direct_redo"]["total_ms"], (h["profile"], r["profile"])


def test_the_step_is_four_launches(arms):
    """the library's profile of ONE 1024-blob call: parse, accumulate, second pass, tail -- no fold and no finalize launch of their own;
    the other arm keeps the five kernels of before"""
    new, old = arms[1]["profile_1024"], arms[0]["profile_1024"]
    assert sorted(new) == ["k_commit_tail", "k_direct_accumulate_asm", "k_direct_redo", "k_parse_be_reduce"], new
    assert all(v["launches"] == 1 for v in new.values()), new
    assert sorted(old) == ["k_direct_accumulate_asm", "k_direct_fold_lanes", "k_direct_redo", "k_finalize_compress", "k_parse_be_reduce"], old
