// cells_verify_host.h -- the host's decisions of a cell proof verification that says where its faults are, on plain blocks: the first
// fault and the code, or r (first_fault, decide_or_challenge); r's bytes (cell_r_bytes); the two host steps of a GROUPED call
// (groups_decide, groups_answers). ONE piece of code for the synchronous grouped call (cells_verify_groups.hip),
// the cell verifier's host functions and the two *_host_steps hooks (cells_verify_async.hip; sections 4n, 4r), through which the tests
// reach all of it without a GPU. It keeps to the rules of a host function (async_verifier.h): no HIP call, no lock held across a wait
// for the GPU, no set_error; cell_batch_finish forks by SideTask, never by host_parallel_for, so the pairings may run in the pool's jobs.
#pragma once
#include "async_verifier.h"      // kNoneBad
#include "cell_groups_plan.h"    // kPwWords
#include "cells_common.h"        // bad_input; engine.h: Fr and cell_batch_challenge / _powers / _finish, which is what keeps HIP's types here

#include <functional>

namespace lwk {

void host_parallel_for(size_t n, const std::function<void(size_t)> &fn);  // sha256_host.hip: persistent workers

// the lowest item at fault: an item's own word (a cell element, its proof), or a distinct commitment's at the item it was first seen at.
// fault: the n items' words; fault_c: the m distinct commitments' (fault + n in a batch call; a group of a grouped call has its slices
// of the call's two runs of words, and first_item then counts in the call's items). first_item == nullptr: the caller asks whether, not
// where -- a commitment at fault then counts at item 0
inline uint32_t first_fault(const int32_t *fault, const int32_t *fault_c, const uint32_t *first_item, size_t n, size_t m) {
    uint32_t bad = kNoneBad;
    for (size_t i = 0; i < n; i++)
        if (fault[i] != 0) {
            bad = (uint32_t)i;
            break;
        }
    for (size_t j = 0; j < m; j++)
        if (fault_c[j] != 0) {
            const uint32_t at = first_item ? first_item[j] : 0u;
            if (at < bad) bad = at;
        }
    return bad;
}

// The code and first_bad of a rejected batch, or r into r_raw and true. bad_index: the lowest i with an index >= 128 (kNoneBad: none),
// decided first, whatever else is wrong
inline bool decide_or_challenge(uint32_t r_raw[8], uint32_t *first_bad, int32_t *rc, const uint8_t *distinct48, size_t m, const uint8_t *digests32,
                                size_t n, uint32_t bad_index, const int32_t *fault, const int32_t *fault_c, const uint32_t *first_item, int mode) {
    if (bad_index != kNoneBad) {
        *first_bad = bad_index;
        *rc = C_KZG_BADARGS;
        return false;
    }
    *first_bad = first_fault(fault, fault_c, first_item, n, m);
    if (*first_bad != kNoneBad) {
        *rc = bad_input(mode);
        return false;
    }
    cell_batch_challenge(r_raw, distinct48, m, digests32, n, mode_rules(mode).little_endian);
    return true;
}

// r as the partials and lwkzg_cell_batch_challenge_host give it: 32 bytes in the mode's byte order
inline void cell_r_bytes(uint8_t out32[32], const uint32_t r_raw[8], int mode) {
    if (mode_rules(mode).little_endian) raw_to_le<8>(out32, r_raw);
    else raw_to_be<8>(out32, r_raw);
}

// ---- a grouped call's two host steps -----------------------------------------------------------------------------------------------------
inline const uint8_t *at_byte(const uint8_t *p, size_t off) { return p ? p + off : nullptr; }

// Step 1. Per group decide_or_challenge on the group's own slices of the call's arrays, then its powers: rc[j] the group's code so far,
// r_raw[8 j] its r, pw[33 j] its power table, flags[j] = 1 for a group nothing behind r is to run for (empty, a bad index, a fault).
// off: the call's g + 1 offsets; gbad[j] != 0: an index of group j is not below 128; fault: 2 n words (items, then concatenated rows);
// first_item (nullptr: see first_fault), distinct48: by concatenated row
inline void groups_decide(int32_t *rc, uint32_t *r_raw, Fr *pw, uint32_t *flags, const uint32_t *off, size_t g, size_t n, const uint32_t *row_base,
                          const uint32_t *gbad, const int32_t *fault, const uint32_t *first_item, const uint8_t *digests32,
                          const uint8_t *distinct48, int mode) {
    host_parallel_for(g, [&](size_t j) {
        const uint32_t lo = off[j], cnt = off[j + 1] - lo;
        flags[j] = 1;
        rc[j] = (int32_t)C_KZG_OK;
        if (cnt == 0) return;   // the batch call's answer to n == 0
        const bool dead = gbad[j] != 0;
        const uint32_t rb = dead ? 0 : row_base[j], m = dead ? 0 : row_base[j + 1] - rb;
        if (!dead && (m == 0 || m > cnt)) {   // (the grouping left no such group)
            rc[j] = (int32_t)C_KZG_ERROR;
            return;
        }
        uint32_t first_bad;
        if (!decide_or_challenge(r_raw + 8 * j, &first_bad, &rc[j], at_byte(distinct48, 48 * (size_t)rb), m, at_byte(digests32, 32 * (size_t)lo),
                                 cnt, dead ? 0u : kNoneBad, fault ? fault + lo : nullptr, fault ? fault + n + rb : nullptr,
                                 first_item ? first_item + rb : nullptr, mode))
            return;
        cell_batch_powers(pw + kPwWords * j, r_raw + 8 * j);
        flags[j] = 0;
    });
}

// Step 2. A group without a flag takes cell_batch_finish on its three sums and RLI, and rc[j] becomes that call's code; then group j's
// answer -- rc[j], and ok where the pairing holds or the group is empty -- and its partials (zero bytes for a flagged group and for
// one whose finish fails). sums_of(j, sums, infs, rli48): the sums where the caller keeps them; false: not well formed.
// ok_out == rc_out == nullptr: the partials alone, and no pairing runs
template <class SumsOf>
void groups_answers(uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out, int32_t *rc, const uint32_t *r_raw, const uint32_t *flags,
                    const uint32_t *off, size_t g, const KZGSettings *s, int mode, const SumsOf &sums_of) {
    constexpr size_t kPart = LWKZG_CELL_VERIFY_PARTIAL_BYTES;
    const bool answers = ok_out && rc_out;
    host_parallel_for(g, [&](size_t j) {
        uint8_t *part = partials_out ? partials_out + kPart * j : nullptr;
        bool ok = off[j + 1] == off[j];
        if (!flags[j]) {
            try {
                uint8_t sums[3][96], rli48[48];
                int infs[3];
                if (part) cell_r_bytes(part, r_raw + 8 * j, mode);
                rc[j] = sums_of(j, sums, infs, rli48) ? cell_batch_finish(answers ? &ok : nullptr, part ? part + 32 : nullptr, sums, infs, rli48, s)
                                                      : C_KZG_BADARGS;
            } catch (...) {
                rc[j] = C_KZG_ERROR;
            }
        }
        if (part && (flags[j] || rc[j] != (int32_t)C_KZG_OK)) memset(part, 0, kPart);
        if (answers) rc_out[j] = rc[j], ok_out[j] = rc[j] == (int32_t)C_KZG_OK && ok ? 1 : 0;
    });
}

}  // namespace lwk
