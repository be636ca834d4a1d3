// cell_group.cuh -- what the grouping kernels of a cell proof batch (cell_group.hip) share with the host: the keyed
// slot hash of a 48-byte commitment, the byte compare, and the size of the table. Compiled for host and device, so that
// tests/cell_group_check.hip runs the same hash and compare through a sequential emulation of the kernels against a plain map.
//
// The table is open addressing over item indices: a slot holds kGroupEmpty or the index of an item whose 48 bytes are the slot's key.
// The inputs are gossip: with a fixed hash a peer could craft commitments that share one probe chain and make the insertion quadratic,
// so the hash is SipHash-2-4 under a 64-bit seed that every verifier draws at creation (k0 = seed, k1 = a fixed mix of it).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LWK_GROUP_HD __host__ __device__ __forceinline__
#else
#define LWK_GROUP_HD inline
#endif

namespace lwk {

constexpr uint32_t kGroupEmpty = 0xffffffffu;   // an empty slot; also "no bad index"
constexpr uint32_t kGroupColumns = 128;         // cells per blob: the bins of the column list

// slots of the table for a verifier of `cap` items: at least 2 cap, a power of two (never more than half full: every probe chain ends)
inline size_t group_table_slots(size_t cap) {
    size_t s = 64;
    while (s < 2 * cap) s <<= 1;
    return s;
}

LWK_GROUP_HD uint64_t group_rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

LWK_GROUP_HD void group_sipround(uint64_t &v0, uint64_t &v1, uint64_t &v2, uint64_t &v3) {
    v0 += v1;
    v1 = group_rotl(v1, 13);
    v1 ^= v0;
    v0 = group_rotl(v0, 32);
    v2 += v3;
    v3 = group_rotl(v3, 16);
    v3 ^= v2;
    v0 += v3;
    v3 = group_rotl(v3, 21);
    v3 ^= v0;
    v2 += v1;
    v1 = group_rotl(v1, 17);
    v1 ^= v2;
    v2 = group_rotl(v2, 32);
}

// the six 64-bit words of a commitment (48 i is a multiple of 8: the words are aligned whenever the array is)
LWK_GROUP_HD void group_load48(uint64_t w[6], const uint8_t *key48) {
    const uint64_t *p = (const uint64_t *)key48;
#pragma unroll
    for (int k = 0; k < 6; k++) w[k] = p[k];
}

// SipHash-2-4 of the six words under (seed, mix(seed)), folded to 32 bits and ANDed with hash_mask (0xffffffff outside the tests:
// mask 0 puts every key on one chain). The caller reduces it to the table.
LWK_GROUP_HD uint32_t group_slot_hash(const uint64_t w[6], uint64_t seed, uint32_t hash_mask) {
    const uint64_t k0 = seed, k1 = (seed ^ 0x9e3779b97f4a7c15ull) * 0xbf58476d1ce4e5b9ull + 0x94d049bb133111ebull;
    uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = k0 ^ 0x6c7967656e657261ull, v3 = k1 ^ 0x7465646279746573ull;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        v3 ^= w[k];
        group_sipround(v0, v1, v2, v3);
        group_sipround(v0, v1, v2, v3);
        v0 ^= w[k];
    }
    const uint64_t last = (uint64_t)48 << 56;   // the length byte of the (empty) tail block
    v3 ^= last;
    group_sipround(v0, v1, v2, v3);
    group_sipround(v0, v1, v2, v3);
    v0 ^= last;
    v2 ^= 0xff;
#pragma unroll
    for (int k = 0; k < 4; k++) group_sipround(v0, v1, v2, v3);
    const uint64_t h = v0 ^ v1 ^ v2 ^ v3;
    return (uint32_t)(h ^ (h >> 32)) & hash_mask;
}

// the slot hash of a SEGMENTED grouping (a call of g groups: the key is (group, 48 bytes)): the same keyed hash
// with the group mixed into both halves of the key, so that one commitment in two groups starts two unrelated probe chains
LWK_GROUP_HD uint32_t group_slot_hash_seg(const uint64_t w[6], uint32_t group, uint64_t seed, uint32_t hash_mask) {
    const uint64_t g = ((uint64_t)group + 1) * 0xd6e8feb86659fd93ull;
    return group_slot_hash(w, seed ^ g ^ (g >> 29), hash_mask);
}

LWK_GROUP_HD bool group_equal48(const uint64_t a[6], const uint8_t *other48) {
    const uint64_t *p = (const uint64_t *)other48;
    uint64_t d = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) d |= a[k] ^ p[k];
    return d == 0;
}

}  // namespace lwk
