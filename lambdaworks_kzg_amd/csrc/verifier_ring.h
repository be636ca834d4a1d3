// verifier_ring.h -- the job slots of an asynchronous verifier (async_verifier.h: verify_async.hip, cells_verify_async.hip), their
// hand-over and the protocol of an enqueue, free of any device code.
//
// Two kinds of thread meet here. The ENQUEUING thread (a caller of lwkzg_verifier_enqueue) takes a slot for its call: `acquire`, which
// waits only when `Depth` calls are already in flight -- the one place an enqueue may block. The RUNTIME's callback thread, which runs
// the call's host functions in stream order, fills the caller's result, completes it (`complete_now`: the state word is stored LAST,
// with release order, so that whoever reads state == 1 with acquire order -- or behind a stream that was ordered after the call -- sees
// the whole result) and gives the slot back (`release`). `pending` and `wait` are for either side's observers.
//
// The mutex guards the ring's own few words and is never held across anything that waits for a stream or an event, nor while a job's
// work runs: a host function that takes it cannot be kept waiting by a thread that is itself waiting for the GPU. Plain C++ so that the
// same code runs on a CPU under -fsanitize=thread (tests/verifier_ring_tsan.cpp, tests/test_verify_async_cpu.py).
#pragma once
#include <condition_variable>
#include <mutex>
#include <stdint.h>

namespace lwk {

// Job: anything default-constructible; the ring hands out pointers into its own array and never looks inside.
template <class Job, int Depth>
struct VerifierRing {
    std::mutex m;
    std::condition_variable cv;
    Job slots[Depth];
    bool busy[Depth] = {};
    int in_flight = 0;
    uint64_t issued = 0;   // calls that were given a slot, ever: a job's ticket (acquire's *ticket) is its place in the verifier's order

    // enqueuing thread: a free slot, waiting for the oldest call in flight to complete when there is none
    Job *acquire(uint64_t *ticket = nullptr) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return in_flight < Depth; });
        int k = 0;
        while (busy[k]) k++;
        busy[k] = true;
        in_flight++;
        if (ticket) *ticket = issued;
        issued++;
        return &slots[k];
    }

    // runtime's thread, once the result is filled in: the state word last (complete_now below does both); and its reader
    static void publish(int32_t *state) { __atomic_store_n(state, 1, __ATOMIC_RELEASE); }
    static bool complete(const int32_t *state) { return __atomic_load_n(state, __ATOMIC_ACQUIRE) == 1; }

    // runtime's thread behind complete_now (or the enqueuing thread, for a call that failed before host function 2 was handed over)
    void release(Job *j) {
        std::lock_guard<std::mutex> lk(m);
        busy[j - slots] = false;
        in_flight--;
        cv.notify_all();   // under the lock: a waiter that sees in_flight == 0 may destroy the ring as soon as it has the mutex
    }

    int pending() {
        std::lock_guard<std::mutex> lk(m);
        return in_flight;
    }

    void wait() {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return in_flight == 0; });
    }
};

// A result (LwkzgVerifyResult, LwkzgCellVerifyResult: state, rc, ok) is final: rc and ok, the state word last
template <class Res>
void complete_now(Res *res, int rc, bool ok) {
    res->rc = (int32_t)rc;
    res->ok = ok ? 1 : 0;
    __atomic_store_n(&res->state, 1, __ATOMIC_RELEASE);
}

// One call's way into the stream. fill(job) writes the acquired slot; enqueue(job, &hf) hands the work over, keeps in hf the number of
// host functions the runtime has taken so far (0, 1 or 2: the second one completes the result and releases the slot itself) and returns
// 0 for success; drain() returns once everything handed over has run. A FAILING enqueue, and only that: whatever was handed over runs
// before the slot and the result are touched again, and they are touched only where host function 2 will not do it -- a slot released
// twice takes in_flight below zero, one never released parks the verifier for good at depth. Returns 0 or error_rc: codes are plain
// integers here.
template <class Ring, class Res, class Fill, class Enqueue, class Drain>
int ring_enqueue(Ring &ring, Res *res, int error_rc, Fill fill, Enqueue enqueue, Drain drain) {
    auto *j = ring.acquire();   // the one place a call may wait: Depth calls are in flight
    fill(j);
    int hf = 0;
    if (enqueue(j, &hf) == 0) return 0;
    if (hf) drain();
    if (hf < 2) {   // (behind host function 2 the result is complete and the slot free already)
        complete_now(res, error_rc, false);
        ring.release(j);
    }
    return error_rc;
}

}  // namespace lwk
