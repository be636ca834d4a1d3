// The job slots of an asynchronous verifier and the protocol of an enqueue (lambdaworks_kzg_amd/csrc/verifier_ring.h: VerifierRing,
// ring_enqueue) on a CPU under -fsanitize=thread: several producer threads play callers of lwkzg_verifier_enqueue, ONE consumer thread
// plays the runtime's callback thread that runs the host functions in stream order. The "stream" is a queue between them; a call hands
// it two stages (host function 1, host function 2), and "drain" -- hipStreamSynchronize in the library -- waits until it is empty.
// Three calls in ten FAIL after handing over 0, 1 or 2 stages. Checked: never more than Depth jobs in flight; every job that reached
// stage 2 is completed there exactly once and in the order it was handed to the stream; a call that failed before stage 2 is completed
// by the protocol with the error code, behind whatever it had handed over; one that failed behind stage 2 keeps stage 2's verdict; no
// slot is released twice; drain runs for failures with something handed over and for nothing else; a result's fields are visible to
// whoever reads state == 1; pending() and wait() agree with that; far more enqueues than slots.
//
// usage: verifier_ring_tsan <producers> <calls per producer>; prints "<n> jobs, <k> check failures"
#include "verifier_ring.h"

#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include <vector>

namespace {

constexpr int kDepth = 4;
constexpr int kErr = 2;   // the code a failed enqueue completes its result with

struct Result {
    int32_t state = 0;
    int32_t rc = -1;
    int32_t ok = 0;
    uint64_t stage1 = 0;      // written by stage 1
    uint64_t payload = 0;     // written by stage 2 before state, read after it
    uint64_t order = 0;       // the consumer's count when it completed this one
};

struct Job {
    Result *res = nullptr;
    uint64_t seq = 0, payload = 0;   // seq: the job's place among those handed to stage 2
};

std::atomic<int> failures{0};
void check(bool ok, const char *what) {
    if (!ok) {
        failures++;
        fprintf(stderr, "check failed: %s\n", what);
    }
}

struct Ring : lwk::VerifierRing<Job, kDepth> {   // counts what the protocol and the consumer do to each slot
    typedef lwk::VerifierRing<Job, kDepth> Base;
    std::atomic<uint64_t> acquires[kDepth] = {}, releases[kDepth] = {};
    Job *acquire() {
        Job *j = Base::acquire();
        acquires[j - slots]++;
        return j;
    }
    void release(Job *j) {
        check(++releases[j - slots] == acquires[j - slots].load(), "a slot is released once per acquire");
        Base::release(j);
    }
};

struct Stream {   // what hipLaunchHostFunc is to the verifier: stages run one at a time, in the order they were handed over
    std::mutex m;
    std::condition_variable cv, idle;
    std::deque<std::pair<Job *, int>> q;
    bool running = false, closed = false;
    void push(Job *j, int stage) {
        {
            std::lock_guard<std::mutex> lk(m);
            q.emplace_back(j, stage);
        }
        cv.notify_one();
    }
    void drain() {
        std::unique_lock<std::mutex> lk(m);
        idle.wait(lk, [&] { return q.empty() && !running; });
    }
};

// how the call k of producer p goes: -1 succeeds, 0 / 1 / 2 fails with that many stages handed over
int plan_of(int p, int k) {
    const int h = (p * 131 + k * 7919) % 10;
    return h < 3 ? h : -1;
}

}  // namespace

int main(int argc, char **argv) {
    const int producers = argc > 1 ? atoi(argv[1]) : 6, calls = argc > 2 ? atoi(argv[2]) : 200;
    Ring ring;
    Stream st;
    std::mutex enq_mu;   // the verifier's: one enqueue at a time, so that hand-over order is the order of the calls
    uint64_t handed = 0; // jobs handed to stage 2 (under enq_mu)
    std::vector<std::vector<Result>> results(producers, std::vector<Result>(calls));
    std::atomic<uint64_t> completed{0}, drains{0}, want_completed{0}, want_drains{0};

    std::thread consumer([&] {
        uint64_t next_seq = 0, done = 0;
        for (;;) {
            Job *j;
            int stage;
            {
                std::unique_lock<std::mutex> lk(st.m);
                st.cv.wait(lk, [&] { return !st.q.empty() || st.closed; });
                if (st.q.empty()) break;
                j = st.q.front().first;
                stage = st.q.front().second;
                st.q.pop_front();
                st.running = true;
            }
            Result *r = j->res;
            check(ring.pending() >= 1 && ring.pending() <= kDepth, "pending within 1 .. Depth while a job runs");
            check(!Ring::complete(&r->state), "a job is completed once, and not before its stages ran");
            if (stage == 1) {
                r->stage1 = j->payload;
            } else {
                check(j->seq == next_seq, "jobs complete in the order they were handed over");
                next_seq++;
                check(r->stage1 == j->payload, "stage 2 runs behind stage 1");
                r->payload = j->payload;
                r->order = done++;
                lwk::complete_now(r, 0, true);   // state last
                completed++;
                ring.release(j);
            }
            {
                std::lock_guard<std::mutex> lk(st.m);
                st.running = false;
            }
            st.idle.notify_all();
        }
    });

    std::vector<std::thread> threads;
    for (int p = 0; p < producers; p++)
        threads.emplace_back([&, p] {
            for (int k = 0; k < calls; k++) {
                Result *r = &results[p][k];
                const uint64_t payload = ((uint64_t)p << 32) | (uint64_t)k | (1ull << 63);
                const int plan = plan_of(p, k);
                {
                    std::lock_guard<std::mutex> enq(enq_mu);
                    const int rc = lwk::ring_enqueue(
                        ring, r, kErr,
                        [&](Job *j) {   // waited while kDepth were in flight
                            check(ring.pending() <= kDepth, "never more than Depth in flight");
                            j->res = r;
                            j->payload = payload;
                        },
                        [&](Job *j, int *hf) {
                            if (plan == 0) return 1;
                            st.push(j, 1);
                            *hf = 1;
                            if (plan == 1) return 1;
                            j->seq = handed++;
                            st.push(j, 2);
                            *hf = 2;
                            return plan == 2 ? 1 : 0;
                        },
                        [&] {
                            drains++;
                            st.drain();
                        });
                    check(rc == (plan < 0 ? 0 : kErr), "the call returns 0, or the error code when its enqueue failed");
                    if (plan == 0 || plan == 1) {   // completed by the protocol, behind what was handed over; the slot is free again
                        check(Ring::complete(&r->state) && r->rc == kErr && r->ok == 0 && r->payload == 0, "a failed call is complete with the error code");
                        check(r->stage1 == (plan == 1 ? payload : 0), "a failed call's stages ran before its result was touched");
                    }
                    if (plan == 2)
                        check(Ring::complete(&r->state) && r->rc == 0 && r->ok == 1 && r->payload == payload, "behind stage 2 the verdict is stage 2's");
                    if (plan != 0 && plan != 1) want_completed++;
                    if (plan >= 1) want_drains++;
                }
                if (k % 7 == 0) {   // a caller that polls its result
                    while (!Ring::complete(&r->state)) std::this_thread::yield();
                    check(plan == 0 || plan == 1 ? r->rc == kErr : r->payload == payload && r->rc == 0, "the result is whole behind state == 1");
                }
                if (k % 31 == 0) {  // a caller that waits for everything (other producers may enqueue meanwhile: only its own are certain)
                    ring.wait();
                    check(Ring::complete(&r->state), "wait() returns behind the caller's own jobs");
                }
            }
        });
    for (auto &t : threads) t.join();
    ring.wait();
    check(ring.pending() == 0, "nothing pending after wait()");
    {
        std::lock_guard<std::mutex> lk(st.m);
        st.closed = true;
    }
    st.cv.notify_all();
    consumer.join();
    const uint64_t n = (uint64_t)producers * (uint64_t)calls;
    check(ring.issued == n, "every call was given a slot");
    check(completed.load() == want_completed.load() && handed == want_completed.load(), "every job handed to stage 2 was completed there");
    check(drains.load() == want_drains.load(), "drain runs for a failure with something handed over, and only then");
    uint64_t acquired = 0, released = 0;
    for (int s = 0; s < kDepth; s++) {
        acquired += ring.acquires[s].load();
        released += ring.releases[s].load();
        check(!ring.busy[s], "no slot is left taken");
    }
    check(acquired == n && released == n && ring.in_flight == 0, "every slot was released exactly once");
    std::vector<char> seen(n, 0);
    for (int p = 0; p < producers; p++) {
        const Result *before = nullptr;   // the producer's previous job that stage 2 completed
        for (int k = 0; k < calls; k++) {
            const Result &r = results[p][k];
            const uint64_t payload = ((uint64_t)p << 32) | (uint64_t)k | (1ull << 63);
            const int plan = plan_of(p, k);
            if (plan == 0 || plan == 1) {
                check(r.state == 1 && r.rc == kErr && r.ok == 0 && r.payload == 0, "a failed call's result holds the error code");
                continue;
            }
            check(r.state == 1 && r.rc == 0 && r.ok == 1 && r.payload == payload, "a result belongs to its own job");
            check(r.order < n && !seen[r.order], "exactly once");
            if (r.order < n) seen[r.order] = 1;
            if (before) check(before->order < r.order, "a producer's jobs complete in its own order");
            before = &r;
        }
    }
    printf("%llu jobs, %d check failures\n", (unsigned long long)n, failures.load());
    return failures.load() ? 1 : 0;
}
