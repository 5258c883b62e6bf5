// Host check of the multi-stream counter-mode plan (csrc/ctr_plan.hpp: ctr_flatten, ctr_plan_multi): the groups
// are pairwise distinct (slot, position, value) triples, every (block, position) maps to the group that holds that
// block's slot and byte, streams of one slot share groups and streams of different slots share none, and each
// block carries its place in the concatenated output.  Built plain and with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>

#include "../../tfhe-aes-2_amd/csrc/ctr_plan.hpp"

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

static tae::CtrStream stream(int32_t slot, const uint8_t iv[8], uint64_t first, size_t len) {
    tae::CtrStream s;
    s.slot = slot;
    for (int p = 0; p < 8; p++) s.iv[p] = iv[p];
    s.first_counter = first;
    s.len = len;
    return s;
}

// plans the streams in chunks of `chunk` blocks and checks every chunk; returns the groups of the whole call
static size_t check_streams(const std::vector<tae::CtrStream> &streams, int64_t n_keys, size_t chunk) {
    std::vector<tae::CtrBlock> blocks;
    CHECK(tae::ctr_flatten(streams.data(), streams.size(), n_keys, blocks) == tae::CTR_FLAT_OK);
    // the flattened list against the streams: order, counters, output places and lengths
    size_t at = 0, out = 0;
    for (const tae::CtrStream &s : streams) {
        const size_t nb = (s.len + 15) / 16;
        for (size_t i = 0; i < nb; i++, at++) {
            CHECK(at < blocks.size());
            if (at >= blocks.size()) return 0;
            const tae::CtrBlock &b = blocks[at];
            CHECK(b.slot == s.slot && b.counter == s.first_counter + i);
            CHECK(b.out_byte == (int64_t)(out + 16 * i));
            CHECK(b.len == (int32_t)(i + 1 < nb ? 16 : s.len - 16 * i) && b.len >= 1 && b.len <= 16);
            for (int p = 0; p < 8; p++) CHECK(b.iv[p] == s.iv[p]);
        }
        out += s.len;
    }
    CHECK(at == blocks.size());
    for (size_t b0 = 0; b0 < blocks.size(); b0 += chunk) {
        const size_t n = std::min(chunk, blocks.size() - b0);
        tae::CtrPlanMulti plan;
        tae::ctr_plan_multi(blocks.data() + b0, n, plan);
        CHECK(plan.map.size() == n * 16 && plan.block_slot.size() == n && plan.block_out.size() == n &&
              plan.block_len.size() == n && plan.group_slot.size() == plan.groups.size());
        std::set<std::tuple<int32_t, int, int>> uniq, want;
        for (size_t g = 0; g < plan.groups.size(); g++)
            uniq.insert(std::make_tuple(plan.group_slot[g], plan.groups[g] >> 8, plan.groups[g] & 0xff));
        CHECK(uniq.size() == plan.groups.size());  // pairwise distinct
        for (size_t i = 0; i < n; i++) {
            const tae::CtrBlock &b = blocks[b0 + i];
            CHECK(plan.block_slot[i] == b.slot && plan.block_out[i] == b.out_byte && plan.block_len[i] == b.len);
            for (int pos = 0; pos < 16; pos++) {
                const uint8_t v = pos < 8 ? b.iv[pos] : (uint8_t)(b.counter >> (8 * (15 - pos)));
                const int32_t g = plan.map[i * 16 + pos];
                CHECK(g >= 0 && (size_t)g < plan.groups.size());
                if (g < 0 || (size_t)g >= plan.groups.size()) continue;
                CHECK(plan.group_slot[g] == b.slot && plan.groups[g] == (uint16_t)((pos << 8) | v));
                want.insert(std::make_tuple(b.slot, pos, (int)v));
            }
        }
        CHECK(want == uniq);  // no group that no block uses
    }
    tae::CtrPlanMulti whole;
    tae::ctr_plan_multi(blocks.data(), blocks.size(), whole);
    return whole.groups.size();
}

int main() {
    const uint8_t iv[8] = {0xbd, 0xd2, 0x19, 0xb8, 0xa0, 0x8d, 0xed, 0x1a};
    uint8_t iv2[8];
    for (int p = 0; p < 8; p++) iv2[p] = (uint8_t)~iv[p];
    CHECK(check_streams({stream(0, iv, 1, 48)}, 1, 1024) == 18);
    CHECK(check_streams({stream(0, iv, 1, 48), stream(1, iv, 1, 48)}, 2, 1024) == 36);
    CHECK(check_streams({stream(0, iv, 1, 48), stream(0, iv, 2, 48)}, 1, 1024) == 19);  // 8 + 7 + 4
    CHECK(check_streams({stream(0, iv, 1, 48), stream(0, iv2, 1, 48)}, 1, 1024) == 26);  // its own 8 iv groups
    CHECK(check_streams({stream(0, iv, 1, 48), stream(0, iv, 9, 0)}, 1, 1024) == 18);    // len 0 adds nothing
    CHECK(check_streams({}, 0, 1024) == 0);
    // about 40 blocks over three slots: partial last blocks, a carry into byte 14, a chunk boundary inside streams
    const std::vector<tae::CtrStream> big = {stream(2, iv, 250, 16 * 13 + 5), stream(0, iv2, 1, 16 * 12),
                                             stream(1, iv, 250, 16 * 9 + 1), stream(2, iv, 255, 16 * 5 + 15)};
    const size_t u = check_streams(big, 3, 1024);
    CHECK(check_streams(big, 3, 7) == u);
    CHECK(check_streams(big, 3, 1) == u);
    // slot 2: iv 8, bytes 8..13 6, byte 14 {0, 1} 2, byte 15: 250..263 -> 14 values = 30;
    // slot 0: 8 + 7 + 12 = 27; slot 1: 8 + 6 + 2 + 10 = 26
    CHECK(u == 30 + 27 + 26);
    // errors leave no blocks
    std::vector<tae::CtrBlock> blocks(3);
    const tae::CtrStream wrap = stream(0, iv, UINT64_MAX, 17), neg = stream(-1, iv, 1, 1), high = stream(2, iv, 1, 1);
    CHECK(tae::ctr_flatten(&wrap, 1, 1, blocks) == tae::CTR_FLAT_WRAP && blocks.empty());
    CHECK(tae::ctr_flatten(&neg, 1, -1, blocks) == tae::CTR_FLAT_SLOT);
    CHECK(tae::ctr_flatten(&high, 1, 2, blocks) == tae::CTR_FLAT_SLOT);
    CHECK(tae::ctr_flatten(&high, 1, -1, blocks) == tae::CTR_FLAT_OK && blocks.size() == 1);
    const tae::CtrStream last = stream(0, iv, UINT64_MAX, 16);
    CHECK(tae::ctr_flatten(&last, 1, 1, blocks) == tae::CTR_FLAT_OK && blocks.size() == 1);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
