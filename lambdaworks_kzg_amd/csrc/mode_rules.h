// mode_rules.h -- what a semantics mode MEANS, in one place. The entry points and the engine ask these questions; none of them compares a
// mode with LWKZG_MODE_CKZG or LWKZG_MODE_REFERENCE itself (DESIGN.md section 4o has the table).
//
//                                  reference                     c-kzg                        eth (consensus specs)
//   a blob stands for              monomial coefficients         evaluations, bit-reversed    evaluations, bit-reversed
//   bytes of elements / z / y      big-endian                    little-endian                big-endian
//   element / z / y not below r    reduced                       rejected                     rejected
//   transcript's integer fields    le64(4096) le64(0) | le64     the same                     be128(4096) | be64
//   digest -> field element        big-endian, reduced           little-endian, reduced       big-endian, reduced
//   rejection code / empty batch   C_KZG_ERROR / false           C_KZG_BADARGS / true         C_KZG_BADARGS / true
#pragma once
#include "../../include/lambdaworks_kzg_amd.h"

namespace lwk {

// How a kernel reads a caller's 32-byte scalar (z, y, a blob element where the kernel takes a rule): the values the `scalar_rule` argument of
// launch_z_from_bytes and launch_each_openings takes, and what the host's fr_from_bytes decides by.
constexpr int kScalarBeReduced = 0;     // big-endian, reduced mod r (reference mode)
constexpr int kScalarLeCanonical = 1;   // little-endian, rejected when not below r (c-kzg mode)
constexpr int kScalarBeCanonical = 2;   // big-endian, rejected when not below r (eth mode)

// What the challenge hash of a blob is told (the `hash_rule` argument of launch_challenge / launch_challenge_finish): bit 0 = the digest is read
// little-endian, bit 1 = the degree field is the consensus specs' be128(4096)
constexpr int kHashDigestLe = 1, kHashFieldsBe = 2;

struct ModeRules {
    bool known;            // one of the LWKZG_MODE_* values
    bool evaluation_form;  // a blob is its polynomial's evaluations on the bit-reversed domain (else: monomial coefficients)
    bool little_endian;    // field elements in and out: blob elements, z, y, cells, challenge outputs, and how a digest is read
    bool canonical;        // an element, z or y that is not below r is rejected (else: reduced)
    bool be_transcript;    // the Fiat-Shamir messages encode their integers big-endian, the blob challenge's degree as 16 bytes
    C_KZG_RET bad;         // what a rejected input answers
    bool empty_ok;         // the verdict of an empty blob batch

    constexpr int le() const { return little_endian ? 1 : 0; }   // the byte order alone: outputs, digests, the cell kernels
    constexpr int scalar_rule() const { return little_endian ? kScalarLeCanonical : canonical ? kScalarBeCanonical : kScalarBeReduced; }
    constexpr int hash_rule() const { return (little_endian ? kHashDigestLe : 0) | (be_transcript ? kHashFieldsBe : 0); }
    // the blob is parsed as reduced monomial coefficients: the parse cannot fail (no verdict word to clear or fetch) and is the kernel that
    // clears the one-blob paths' counters on its way (host_api.hip)
    constexpr bool parse_cannot_fail() const { return !evaluation_form && !canonical; }
    constexpr int bad_status() const { return (int)bad; }         // the status word a kernel writes (plan.h: kStatusBadArgs / kStatusError)
};

constexpr ModeRules mode_rules(int mode) {
    return mode == LWKZG_MODE_ETH    ? ModeRules{true, true, false, true, true, C_KZG_BADARGS, true}
           : mode == LWKZG_MODE_CKZG ? ModeRules{true, true, true, true, false, C_KZG_BADARGS, true}
           : mode == LWKZG_MODE_REFERENCE ? ModeRules{true, false, false, false, false, C_KZG_ERROR, false}
                                          : ModeRules{false, false, false, false, false, C_KZG_ERROR, false};
}
constexpr bool mode_known(int mode) { return mode_rules(mode).known; }

static_assert((int)C_KZG_BADARGS == 1 && (int)C_KZG_ERROR == 2, "the kernels' status words are the ABI's codes");

}  // namespace lwk
