// each.h -- what the per-item verifications share (verify_each.hip: blobs and openings; cells_verify_each.hip: EIP-7594 cells): the
// record an item's pairing check is taken of, its flags, the cached line tables of a context and the launch of k_each_pairing.
#pragma once
#include "engine.h"

namespace lwk {

struct PairingLine;   // fp12.cuh

constexpr int kEachBlock = 64;

// flags of an item: its status was 0 / its P is not the point at infinity / its proof is not the point at infinity
constexpr uint32_t kEachValid = 1, kEachHasP = 2, kEachHasPi = 4;

// the two G1 points of an item's pairing check: P (the blob call's C - [y]G + [z]pi, the cell call's C - [I(tau)]G + [c_k]pi) and -pi, affine
struct alignas(16) EachPoints {
    Fp px, py, qx, qy;
    uint32_t flags;
};

inline unsigned each_blocks(size_t n) { return (unsigned)((n + kEachBlock - 1) / kEachBlock); }

// the line tables of g2_values[0] and g2_values[power] on the device (2 x kPairingLines), kept in *slot (a member of the context, freed
// with it) and made at the first call that wants them. Caller holds the context's mu.
C_KZG_RET each_line_tables(const KZGSettings *s, int power, void **slot, const PairingLine **out);

// ok[i] = e(P_i, G2) e(-pi_i, second G2 point) == 1 for every item whose record is valid, 0 for the others; lines: the pair of tables above
void launch_each_pairing(const EachPoints *pts, const PairingLine *lines, uint8_t *ok, size_t n, hipStream_t st);

}  // namespace lwk
