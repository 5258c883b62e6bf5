// Round-1 plan of AES-128-CTR with public counters (host only, no device code).
//
// Counter block i is iv[8] || be64(first_counter + i) (reference src/bin/main.rs:108-115, which counts
// from 1).  The round-1 SubBytes input of block i at byte position pos is rk0[pos] xor the public byte
// block_i[pos], so it depends on (pos, byte value) alone: every distinct pair is one "group", bootstrapped
// once and shared between the blocks that have it.  Bytes 0..7 (the IV) give one group each, bytes 8..14
// one or two over any realistic run, byte 15 up to 256.
//
// Several streams under several AES keys (ctr_flatten, ctr_plan_multi, below): the round key differs per key
// slot, so a group is a distinct (slot, pos, byte value).
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

// ---- several streams under several keys (a key table) ----
// One counter-mode stream of a multi-key call: len bytes under key slot `slot`, counter blocks
// iv || be64(first_counter + i), i < ceil(len / 16).
struct CtrStream {
    int32_t slot;
    uint8_t iv[8];
    uint64_t first_counter;
    size_t len;
};

// One block of the flattened (stream, block) list, in stream order.  out_byte is the offset of the block's first
// byte in the concatenated output and len (1..16) how many of its bytes the stream has.
struct CtrBlock {
    int32_t slot;
    uint8_t iv[8];
    uint64_t counter;
    int64_t out_byte;
    int32_t len;
};

enum CtrFlatten { CTR_FLAT_OK = 0, CTR_FLAT_SLOT, CTR_FLAT_WRAP };

// Flattens the streams; a stream of len 0 contributes nothing.  n_keys < 0 checks slot >= 0 only.  On an error
// `blocks` is left empty.
inline CtrFlatten ctr_flatten(const CtrStream *streams, size_t n_streams, int64_t n_keys, std::vector<CtrBlock> &blocks) {
    blocks.clear();
    int64_t out = 0;
    for (size_t s = 0; s < n_streams; s++) {
        const CtrStream &st = streams[s];
        if (!st.len) continue;
        const size_t nb = st.len / 16 + (st.len % 16 != 0);
        CtrFlatten err = CTR_FLAT_OK;
        if (st.slot < 0 || (n_keys >= 0 && st.slot >= n_keys)) err = CTR_FLAT_SLOT;
        else if (!ctr_range_ok(st.first_counter, nb)) err = CTR_FLAT_WRAP;
        if (err != CTR_FLAT_OK) {
            blocks.clear();
            return err;
        }
        for (size_t i = 0; i < nb; i++) {
            CtrBlock b;
            b.slot = st.slot;
            for (int p = 0; p < 8; p++) b.iv[p] = st.iv[p];
            b.counter = st.first_counter + i;
            b.out_byte = out + (int64_t)(16 * i);
            b.len = (int32_t)(i + 1 < nb ? 16 : st.len - 16 * i);
            blocks.push_back(b);
        }
        out += (int64_t)st.len;
    }
    return CTR_FLAT_OK;
}

// Round-1 plan of n flattened blocks.  The SubBytes input at (block, pos) is rk0 of the block's slot at pos xor
// the public byte, so a group is a distinct (slot, pos, byte value): streams of one slot share groups, streams
// of different slots share none whatever their public bytes.  groups / group_slot are parallel arrays in
// first-appearance order (blocks in order, positions 0..15 within a block).
struct CtrPlanMulti {
    std::vector<uint16_t> groups;     // (pos << 8) | byte value
    std::vector<int32_t> group_slot;  // the key slot of the group
    std::vector<int32_t> map;         // [n][16]: (block, byte position) -> group index
    std::vector<int32_t> block_slot;  // [n]
    std::vector<int64_t> block_out;   // [n] CtrBlock::out_byte
    std::vector<int32_t> block_len;   // [n] CtrBlock::len
};

inline void ctr_plan_multi(const CtrBlock *blocks, size_t n, CtrPlanMulti &plan) {
    plan = CtrPlanMulti{};
    plan.map.assign(n * 16, 0);
    plan.block_slot.resize(n);
    plan.block_out.resize(n);
    plan.block_len.resize(n);
    // (slot, pos, value) -> group, open addressing on a power-of-two table at most half full
    size_t cap = 64;
    while (cap < n * 32) cap *= 2;
    std::vector<uint64_t> keys(cap, UINT64_MAX);
    std::vector<int32_t> vals(cap, -1);
    for (size_t i = 0; i < n; i++) {
        const CtrBlock &b = blocks[i];
        plan.block_slot[i] = b.slot;
        plan.block_out[i] = b.out_byte;
        plan.block_len[i] = b.len;
        for (int pos = 0; pos < 16; pos++) {
            const uint8_t v = ctr_block_byte(b.iv, b.counter, pos);
            const uint64_t key = ((uint64_t)(uint32_t)b.slot << 16) | (uint64_t)(pos << 8) | v;
            size_t h = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & (cap - 1);
            while (keys[h] != UINT64_MAX && keys[h] != key) h = (h + 1) & (cap - 1);
            if (keys[h] == UINT64_MAX) {
                keys[h] = key;
                vals[h] = (int32_t)plan.groups.size();
                plan.groups.push_back((uint16_t)((pos << 8) | v));
                plan.group_slot.push_back(b.slot);
            }
            plan.map[i * 16 + pos] = vals[h];
        }
    }
}

}  // namespace tae
