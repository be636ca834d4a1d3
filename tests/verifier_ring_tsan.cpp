// The job slots of an asynchronous verifier (lambdaworks_kzg_amd/csrc/verifier_ring.h) on a CPU under -fsanitize=thread: several
// producer threads play callers of lwkzg_verifier_enqueue, ONE consumer thread plays the runtime's callback thread that runs the host
// functions in stream order. The "stream" is a queue between them. Checked: never more than Depth jobs in flight; every job is
// completed exactly once and in the order it was handed to the stream; a result's fields are visible to whoever reads state == 1;
// pending() and wait() agree with that; far more enqueues than slots.
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

struct Result {
    int32_t state = 0;
    int32_t rc = -1;
    uint64_t payload = 0;     // written before state, read after it
    uint64_t order = 0;       // the consumer's count when it completed this one
};

struct Job {
    Result *res = nullptr;
    uint64_t ticket = 0, payload = 0;
};

typedef lwk::VerifierRing<Job, kDepth> Ring;

struct Stream {   // what hipLaunchHostFunc is to the verifier: jobs run one at a time, in the order they were handed over
    std::mutex m;
    std::condition_variable cv;
    std::deque<Job *> q;
    bool closed = false;
};

std::atomic<int> failures{0};
void check(bool ok, const char *what) {
    if (!ok) {
        failures++;
        fprintf(stderr, "check failed: %s\n", what);
    }
}

}  // namespace

int main(int argc, char **argv) {
    const int producers = argc > 1 ? atoi(argv[1]) : 6, calls = argc > 2 ? atoi(argv[2]) : 200;
    Ring ring;
    Stream st;
    std::mutex enq_mu;   // the verifier's: one enqueue at a time, so that ticket order is hand-over order
    std::vector<std::vector<Result>> results(producers, std::vector<Result>(calls));
    std::atomic<uint64_t> completed{0};

    std::thread consumer([&] {
        uint64_t next_ticket = 0, done = 0;
        for (;;) {
            Job *j;
            {
                std::unique_lock<std::mutex> lk(st.m);
                st.cv.wait(lk, [&] { return !st.q.empty() || st.closed; });
                if (st.q.empty()) break;
                j = st.q.front();
                st.q.pop_front();
            }
            check(j->ticket == next_ticket, "jobs complete in the order they were handed over");
            next_ticket++;
            check(ring.pending() >= 1 && ring.pending() <= kDepth, "pending within 1 .. Depth while a job runs");
            Result *r = j->res;
            check(!Ring::complete(&r->state), "a job is completed once");
            r->payload = j->payload;
            r->rc = 0;
            r->order = done++;
            Ring::publish(&r->state);   // state last
            completed++;
            ring.release(j);
        }
    });

    std::vector<std::thread> threads;
    for (int p = 0; p < producers; p++)
        threads.emplace_back([&, p] {
            for (int k = 0; k < calls; k++) {
                Result *r = &results[p][k];
                {
                    std::lock_guard<std::mutex> enq(enq_mu);
                    uint64_t ticket = 0;
                    Job *j = ring.acquire(&ticket);   // waits while kDepth are in flight
                    check(ring.pending() <= kDepth, "never more than Depth in flight");
                    j->res = r;
                    j->ticket = ticket;
                    j->payload = ((uint64_t)p << 32) | (uint64_t)k;
                    {
                        std::lock_guard<std::mutex> lk(st.m);
                        st.q.push_back(j);
                    }
                    st.cv.notify_one();
                }
                if (k % 7 == 0) {   // a caller that polls its result
                    while (!Ring::complete(&r->state)) std::this_thread::yield();
                    check(r->payload == (((uint64_t)p << 32) | (uint64_t)k) && r->rc == 0, "the result is whole behind state == 1");
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
    check(completed.load() == n && ring.issued == n, "every job was completed");
    std::vector<char> seen(n, 0);
    for (int p = 0; p < producers; p++)
        for (int k = 0; k < calls; k++) {
            const Result &r = results[p][k];
            check(r.state == 1 && r.rc == 0 && r.payload == (((uint64_t)p << 32) | (uint64_t)k), "a result belongs to its own job");
            check(r.order < n && !seen[r.order], "exactly once");
            if (r.order < n) seen[r.order] = 1;
            if (k) check(results[p][k - 1].order < r.order, "a producer's jobs complete in its own order");
        }
    printf("%llu jobs, %d check failures\n", (unsigned long long)n, failures.load());
    return failures.load() ? 1 : 0;
}
