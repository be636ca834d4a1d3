"""GPU: the library's profile takes the time of a one-launch scope from the dispatch packet itself (kernels.h: prof_launch -- the launch
carries a pooled start and stop event, nothing else is enqueued) against the arm it replaces (LWKZG_PROF_MARKERS=1: two marker packets on
default-flag events around every launch), in fresh processes. How a launch is timed changes neither what a call computes nor which
launches it makes: the bytes agree between the arms and with an unprofiled call, and so do the names and the launch counts.
tests/dispatch_events_worker.py is what each process runs.

No test here asserts a measured duration beyond two sanity bounds on ONE 512-blob call: the kernels' times add up to no more than the host
clock around the call (synchronize to synchronize), and the accumulation -- over nine tenths of such a call -- is more than half of it. A
zero, an enqueue time or a difference of unrelated timestamps fails one of the two."""
import functools
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FOUR = ["k_commit_tail", "k_direct_accumulate_asm", "k_direct_redo", "k_parse_be_reduce"]
CALLS = ("commit_512", "commit_1", "commit_9", "proofs_16")


@functools.lru_cache(maxsize=None)
def run_arm(arm):
    e = dict(os.environ, LWKZG_EXPERIMENTAL="1", LWKZG_PROF_MARKERS=str(arm))
    e.pop("LWKZG_DIRECT_BITS", None)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tests", "dispatch_events_worker.py")], env=e).decode()
    return json.loads(out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def arms():
    return {arm: run_arm(arm) for arm in (0, 1)}


def _launches(profile):
    return {k: v["launches"] for k, v in profile.items()}


DISABLE_SYSTEM_FENCE, RELEASE_TO_DEVICE = 0x20000000, 0x40000000   # hip_runtime_api.h


def test_the_arms_are_the_arms(arms):
    """by the library's own count of what its profile was made of (lwkzg_profile_sources), not by the knob's echo alone: the shipped arm
    binds EVERY pair of these one-launch calls to a dispatch and records no marker; the other arm records a marker pair for every one.
    The pooled events of the shipped arm carry no system-scope fence; the other arm's have the default flags."""
    assert arms[0]["knob"] == 0 and arms[1]["knob"] == 1
    assert arms[0]["bits"] == arms[1]["bits"] and arms[1]["bits"] >= 10
    for call in ("commit_512", "commit_1", "commit_9"):
        launches = sum(v["launches"] for v in arms[0][call]["profile"].values())
        new, old = arms[0][call]["sources"], arms[1][call]["sources"]
        assert new["dispatch_pairs"] == launches and new["marker_pairs"] == 0 and new["shared_markers"] == 0, (call, new)
        assert old["marker_pairs"] == launches and old["dispatch_pairs"] == 0 and old["shared_markers"] == 0, (call, old)
        assert new["event_flags"] & DISABLE_SYSTEM_FENCE and old["event_flags"] == 0, (new, old)
    print("event flags of the shipped arm: 0x%x" % arms[0]["commit_512"]["sources"]["event_flags"])


def test_back_to_back_marker_scopes_share_one_marker(arms):
    """a per-item verification of four openings: k_decompress_points and k_subgroup_coop_asm are padded launches (possibly two launches each) and
    keep marker scopes; nothing is enqueued between them, so the shipped arm records ONE marker as the first's close and the second's
    open. Same verdicts, names and launch counts in both arms."""
    new, old = arms[0]["openings_4"], arms[1]["openings_4"]
    assert new["verdicts"] == old["verdicts"] == [[[0, True]] * 4] * 2
    assert _launches(new["profile"]) == _launches(old["profile"])
    for k in ("k_decompress_points", "k_subgroup_coop_asm"):
        assert new["profile"][k]["launches"] == 1 and new["profile"][k]["total_ms"] > 0, new["profile"]
    launches = sum(v["launches"] for v in new["profile"].values())
    assert new["sources"]["shared_markers"] == 1 and old["sources"]["shared_markers"] == 0
    assert new["sources"]["dispatch_pairs"] + new["sources"]["marker_pairs"] == launches, new
    assert new["sources"]["marker_pairs"] >= 2 and old["sources"]["marker_pairs"] == launches and old["sources"]["dispatch_pairs"] == 0


@pytest.mark.parametrize("arm", [0, 1])
def test_512_commitments_four_launches_with_sane_times(arms, arm):
    """the smallest call that takes parse, accumulate, second pass and tail: four names, one launch each, every time positive, their sum
    within the host clock around the call and the accumulation more than half of it"""
    r = arms[arm]["commit_512"]
    prof = r["profile"]
    assert sorted(prof) == FOUR, prof
    assert all(v["launches"] == 1 for v in prof.values()), prof
    assert all(v["total_ms"] > 0 for v in prof.values()), prof
    wall = r["on"]["wall_ms"]
    print("arm", arm, "wall_ms", wall, {k: v["total_ms"] for k, v in prof.items()})
    assert sum(v["total_ms"] for v in prof.values()) <= wall, (prof, wall)
    assert prof["k_direct_accumulate_asm"]["total_ms"] > 0.5 * wall, (prof, wall)


@pytest.mark.parametrize("call", CALLS)
def test_results_do_not_depend_on_the_profile(arms, call):
    """byte-equal between the arms and with the unprofiled call of the same inputs; no status word left set"""
    a, b = arms[0][call], arms[1][call]
    assert a["on"]["bytes"] == b["on"]["bytes"] == a["off"]["bytes"] == b["off"]["bytes"]
    assert len(a["on"]["bytes"]) == 96 * int(call.split("_")[1]) and set(a["on"]["bytes"]) != {"0"}
    for r in (a, b):
        assert r["on"]["status_sum"] == 0 and r["off"]["status_sum"] == 0, call


@pytest.mark.parametrize("call", CALLS)
def test_names_and_launch_counts_are_those_of_the_marker_arm(arms, call):
    new, old = arms[0][call]["profile"], arms[1][call]["profile"]
    assert new and _launches(new) == _launches(old), (new, old)
    assert all(v["total_ms"] > 0 for v in new.values()), new


def test_the_small_calls_take_the_paths_they_are_here_for(arms):
    """1 blob: the cooperative kernel; 9 blobs: the hand-scheduled accumulation, the lane fold as its own launch, finalize"""
    one, nine = arms[0]["commit_1"]["profile"], arms[0]["commit_9"]["profile"]
    assert "k_coop_msm_asm" in one and "k_direct_accumulate_asm" not in one, one
    assert all(k in nine for k in ("k_direct_accumulate_asm", "k_direct_fold_lanes", "k_finalize_compress")), nine
    assert "k_commit_tail" not in nine, nine


@pytest.mark.parametrize("arm", [0, 1])
def test_profile_off_reports_nothing(arms, arm):
    for call in CALLS:
        assert arms[arm][call]["report_after_off"] == {}, call


@pytest.mark.parametrize("arm", [0, 1])
def test_pool_reset_while_pending_then_two_calls_in_a_row(arms, arm):
    """a reset while a call's pairs are pending leaves an empty report, not a failure; two profiled calls in a row (the second takes its
    events from the pool) report every launch twice and compute the same bytes"""
    r = arms[arm]
    assert r["report_after_pending_reset"] == {}
    twice = r["twice"]
    assert twice["first"] == twice["second"] == r["commit_9"]["on"]["bytes"]
    assert twice["profile"] and all(v["launches"] == 2 for v in twice["profile"].values()), twice["profile"]
    assert sorted(twice["profile"]) == sorted(r["commit_9"]["profile"])
