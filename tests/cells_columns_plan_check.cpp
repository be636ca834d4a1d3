// The plan of the column calls (lambdaworks_kzg_amd/csrc/cells_columns_plan.h) as a stand-alone program, built under AddressSanitizer
// and UndefinedBehaviorSanitizer by tests/test_cells_columns_cpu.py. Every c in 1 .. 128 x {cells, proofs, both} x {compute, recover}
// x {MSM, FK20 with min_blobs 1, 2, 64} x n_call around every threshold goes through the four functions; what they answer is held
// against the capacities of the workspace written out here on their own (1024 slots of ws.scalars, ws.scalars2 and ws.fr), against
// the full calls' figures at c = 128 and against the host slice's rule. Every case prints one line, "<name> ok" or
// "<name> FAILED: ..."; the exit status is the number of failures.
#include <stdio.h>

#include <string>

#include "cells_columns_plan.h"

using namespace lwk;

namespace {

int failures = 0;

void report(const std::string &name, const std::string &why) {
    if (!why.empty()) failures++;
    printf("%s %s%s\n", name.c_str(), why.empty() ? "ok" : "FAILED:", why.c_str());
}

const size_t kSlots = 1024;   // engine.h: kMaxChunk, written out: the check does not take its bound from the header it checks

std::string at(const ColumnsCall &q, size_t n) {
    return " (c = " + std::to_string(q.c) + (q.cells ? ", cells" : "") + (q.proofs ? ", proofs" : "") + (q.pair_scratch ? ", recover" : "") +
           (q.fk20_on ? ", FK20 from " + std::to_string(q.min_blobs) : "") + ", n = " + std::to_string(n) + ")";
}

// do m blobs of an MSM-path call with proofs fit the workspace?
bool fits(const ColumnsCall &q, size_t m) {
    const bool pair = q.cells || q.pair_scratch;
    return m * q.c <= kSlots && m <= kSlots && (!pair || 2 * m <= kSlots);
}

template <class F>
void every_call(const F &f) {
    for (size_t c = 1; c <= 128; c++)
        for (int outs = 1; outs <= 3; outs++)
            for (int recover = 0; recover < 2; recover++)
                for (size_t min_blobs : {(size_t)0, (size_t)1, (size_t)2, (size_t)64}) {
                    ColumnsCall q;
                    q.c = c, q.cells = outs & 1, q.proofs = outs & 2, q.pair_scratch = recover;
                    q.fk20_on = min_blobs != 0, q.min_blobs = min_blobs;
                    f(q);
                }
}

// n_call around the FK20 threshold of q and around the chunks either engine takes
template <class F>
void every_n(const ColumnsCall &q, const F &f) {
    const size_t edge = q.fk20_on ? (128 * q.min_blobs + q.c - 1) / q.c : 1;   // the first n with n c >= 128 min_blobs
    const size_t around[] = {1, edge, columns_chunk(q, false), columns_chunk(q, true), 64, 1024};
    for (size_t a : around)
        for (size_t n = a > 2 ? a - 2 : 1; n <= a + 2; n++) f(n);
}

void chunk_rule() {
    std::string why;
    every_call([&](const ColumnsCall &q) {
        if (!why.empty()) return;
        const size_t m = columns_chunk(q, false);
        if (!q.proofs) {
            if (m != 512) why = " cells only: a chunk of " + std::to_string(m) + at(q, 0);
            return;
        }
        if (m < 1 || !fits(q, m)) why = " a chunk of " + std::to_string(m) + " breaks a capacity" + at(q, 0);
        else if (fits(q, m + 1)) why = " a chunk of " + std::to_string(m) + " is not the largest" + at(q, 0);
        if (columns_chunk(q, true) != 512) why = " FK20: a chunk of " + std::to_string(columns_chunk(q, true)) + at(q, 0);
    });
    report("chunk: the three capacities hold and m + 1 breaks one", why);
}

void full_call_figures() {
    std::string why;
    for (int outs = 1; outs <= 3 && why.empty(); outs++)
        for (int recover = 0; recover < 2; recover++)
            for (int fk = 0; fk < 2; fk++) {
                ColumnsCall q;
                q.cells = outs & 1, q.proofs = outs & 2, q.pair_scratch = recover, q.fk20_on = fk, q.min_blobs = fk ? 4 : 0;
                for (size_t n : {(size_t)1, (size_t)3, (size_t)4, (size_t)8, (size_t)9, (size_t)511, (size_t)512, (size_t)513, (size_t)5000}) {
                    const bool fk20 = columns_fk20(q, n), was_fk20 = q.proofs && fk && n >= q.min_blobs;   // cells_chunks before the columns
                    const size_t was_chunk = was_fk20 ? 512 : q.proofs ? 8 : 512;
                    const size_t was_reserve = (q.proofs && !was_fk20 ? 128 : 2) * (n < was_chunk ? n : was_chunk);
                    if (fk20 != was_fk20) why = " engine" + at(q, n);
                    else if (columns_chunk(q, fk20) != was_chunk) why = " chunk " + std::to_string(columns_chunk(q, fk20)) + at(q, n);
                    else if (columns_reserve(q, fk20, n) != was_reserve) why = " reserve " + std::to_string(columns_reserve(q, fk20, n)) + at(q, n);
                }
            }
    report("c = 128: 8 / 512 / 512 blobs per chunk and 128 m or 2 m slots, as the full calls have them", why);
}

void reserve_rule() {
    std::string why;
    every_call([&](const ColumnsCall &q) {
        every_n(q, [&](size_t n) {
            if (!why.empty()) return;
            const bool fk20 = columns_fk20(q, n);
            const size_t chunk = columns_chunk(q, fk20), m = n < chunk ? n : chunk, got = columns_reserve(q, fk20, n);
            // what a pass of m blobs touches, in slots: the coefficients, a pair of slots per blob (the extension, the recovery, FK20's
            // scalars), the scalar sets
            size_t need = m;
            if (q.cells || q.pair_scratch || fk20) need = 2 * m;
            if (q.proofs && !fk20 && m * q.c > need) need = m * q.c;
            if (got < need || got > kSlots) why = " " + std::to_string(got) + " slots where " + std::to_string(need) + " are touched" + at(q, n);
            else if (q.proofs && !fk20 && got != need) why = " " + std::to_string(got) + " slots, more than the " + std::to_string(need) + " touched" + at(q, n);
        });
    });
    report("reserve: every slot a pass touches, and no more than a launch set", why);
}

void engine_rule() {
    std::string why;
    every_call([&](const ColumnsCall &q) {
        every_n(q, [&](size_t n) {
            if (!why.empty()) return;
            const bool want = q.proofs && q.fk20_on && n * q.c >= 128 * q.min_blobs;
            if (columns_fk20(q, n) != want) why = " the predicate" + at(q, n);
            if (columns_fk20(q, n) && !columns_fk20(q, n + 1)) why = " not monotone in n" + at(q, n);
            if (q.c < 128) {
                ColumnsCall wider = q;
                wider.c++;
                if (columns_fk20(q, n) && !columns_fk20(wider, n)) why = " not monotone in c" + at(q, n);
            }
        });
    });
    report("engine: FK20 iff it is on, proofs are wanted and n c >= 128 min_blobs; monotone in n and in c", why);
}

void slice_rule() {
    std::string why;
    every_call([&](const ColumnsCall &q) {
        const size_t in_bytes = q.pair_scratch ? 64 * 2048 : 131072;   // a blob, or the least a recovery is given
        const size_t per_blob = in_bytes + (q.cells ? q.c * 2048 : 0) + (q.proofs ? q.c * 48 : 0) + 4;
        every_n(q, [&](size_t n) {
            if (!why.empty()) return;
            const size_t chunk = columns_chunk(q, columns_fk20(q, n)), slice = columns_host_slice(chunk, per_blob, n);
            if (slice < 1 || slice > n) why = " a slice of " + std::to_string(slice) + at(q, n);
            else if (slice != n && slice % chunk != 0) why = " a slice of " + std::to_string(slice) + " is no whole number of chunks of " + std::to_string(chunk) + at(q, n);
            else if (n >= 64 && slice < 64) why = " a slice of " + std::to_string(slice) + " is below the full calls' 64" + at(q, n);
            else if (slice != n && slice > chunk && slice - chunk >= 64 && slice * per_blob > kColumnsStageBytes)
                why = " a slice of " + std::to_string(slice) + " stages more than the bound where fewer chunks would do" + at(q, n);
        });
    });
    report("host slice: whole chunks or the whole call, at least 64 blobs when the call has them, within the staging bound", why);
}

}  // namespace

int main() {
    chunk_rule();
    full_call_figures();
    reserve_rule();
    engine_rule();
    slice_rule();
    return failures;
}
