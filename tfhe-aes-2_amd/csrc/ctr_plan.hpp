// Round-1 plan of AES-128-CTR with public counters (host only, no device code).
//
// Counter block i is iv[8] || be64(first_counter + i) (reference src/bin/main.rs:108-115, which counts
// from 1).  The round-1 SubBytes input of block i at byte position pos is rk0[pos] xor the public byte
// block_i[pos], so it depends on (pos, byte value) alone: every distinct pair is one "group", bootstrapped
// once and shared between the blocks that have it.  Bytes 0..7 (the IV) give one group each, bytes 8..14
// one or two over any realistic run, byte 15 up to 256.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tae {

struct CtrPlan {
    std::vector<uint16_t> groups;  // (pos << 8) | byte value: the 8 IV positions first, then positions
                                   // 8..15, each with its distinct values in first-appearance order
    std::vector<int32_t> map;      // [n_blocks][16]: (block, byte position) -> group index
};

// the counters first_counter .. first_counter + n_blocks - 1 must not wrap past 2^64 - 1
inline bool ctr_range_ok(uint64_t first_counter, size_t n_blocks) {
    return n_blocks == 0 || (uint64_t)(n_blocks - 1) <= UINT64_MAX - first_counter;
}

inline uint8_t ctr_block_byte(const uint8_t iv[8], uint64_t counter, int pos) {
    return pos < 8 ? iv[pos] : (uint8_t)(counter >> (8 * (15 - pos)));
}

// false (plan untouched) when the counter range wraps
inline bool ctr_plan(const uint8_t iv[8], uint64_t first_counter, size_t n_blocks, CtrPlan &plan) {
    if (!ctr_range_ok(first_counter, n_blocks)) return false;
    plan.groups.clear();
    plan.map.assign(n_blocks * 16, 0);
    if (!n_blocks) return true;
    for (int pos = 0; pos < 8; pos++) {
        plan.groups.push_back((uint16_t)((pos << 8) | iv[pos]));
        for (size_t i = 0; i < n_blocks; i++) plan.map[i * 16 + pos] = pos;
    }
    for (int pos = 8; pos < 16; pos++) {
        int32_t seen[256];
        for (int v = 0; v < 256; v++) seen[v] = -1;
        for (size_t i = 0; i < n_blocks; i++) {
            const uint8_t v = ctr_block_byte(iv, first_counter + i, pos);
            if (seen[v] < 0) {
                seen[v] = (int32_t)plan.groups.size();
                plan.groups.push_back((uint16_t)((pos << 8) | v));
            }
            plan.map[i * 16 + pos] = seen[v];
        }
    }
    return true;
}

}  // namespace tae
