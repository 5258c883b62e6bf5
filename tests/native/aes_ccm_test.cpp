// Host check of the CCM layer (csrc/aes_ccm.hpp): ccm_format against RFC 3610 packet vector 1 and at its edges
// (L = 2 and 8, M = 4 and 16, no AAD, AAD of 14 and 15 bytes, payloads of 0, 16 and 17 bytes, every refusal),
// pub_plan (distinct (slot, pos, value) groups, the map inverts, ctr_plan_multi's plan on iv || counter blocks) and
// the two word functions of the chain against plain u64 sums, both byte modes and a partial last block.  Built
// plain and with -fsanitize=address,undefined by tests/test_aes_ccm.py.
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

#include "../../tfhe-aes-2_amd/csrc/aes_ccm.hpp"

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void test_format() {
    // RFC 3610 packet vector 1: nonce 13 bytes (L = 2), AAD 00..07, payload of 23 bytes, M = 8
    const uint8_t nonce[13] = {0x00, 0x00, 0x00, 0x03, 0x02, 0x01, 0x00, 0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5};
    uint8_t aad[16];
    for (int i = 0; i < 16; i++) aad[i] = (uint8_t)i;
    tae::CcmFrame f;
    CHECK(tae::ccm_format(nonce, 13, 8, aad, 8, 23, f) == tae::CCM_FMT_OK);
    CHECK(f.L == 2 && f.M == 8 && f.n_mac() == 4 && f.n_ctr() == 3);
    const uint8_t b0[16] = {0x59, 0x00, 0x00, 0x00, 0x03, 0x02, 0x01, 0x00, 0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5, 0x00, 0x17};
    const uint8_t b1[16] = {0x00, 0x08, 0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0, 0, 0, 0, 0, 0};
    const uint8_t a2[16] = {0x01, 0x00, 0x00, 0x00, 0x03, 0x02, 0x01, 0x00, 0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5, 0x00, 0x02};
    CHECK(!std::memcmp(&f.mac[0], b0, 16) && !std::memcmp(&f.mac[16], b1, 16) && !std::memcmp(&f.ctr[32], a2, 16));
    for (int i = 0; i < 32; i++) CHECK(f.src[i] == -1);
    for (int q = 0; q < 23; q++) CHECK(f.src[32 + q] == q && f.mac[32 + q] == 0);
    for (int i = 32 + 23; i < 64; i++) CHECK(f.src[i] == -1 && f.mac[i] == 0);  // the padding is public zero

    // L = 8 (nonce of 7 bytes), M = 16, no AAD: the Adata flag is clear and no AAD block is made
    CHECK(tae::ccm_format(nonce, 7, 16, nullptr, 0, 16, f) == tae::CCM_FMT_OK);
    CHECK(f.L == 8 && f.n_mac() == 2 && f.n_ctr() == 2);
    CHECK(f.mac[0] == (uint8_t)(8 * 7 + 7) && f.mac[15] == 16 && f.mac[8] == 0 && f.ctr[0] == 7 && f.ctr[16 + 15] == 1);
    for (int q = 0; q < 16; q++) CHECK(f.src[16 + q] == q);
    // M = 4, a payload of 17 bytes: two payload blocks, the second with one byte
    CHECK(tae::ccm_format(nonce, 13, 4, nullptr, 0, 17, f) == tae::CCM_FMT_OK);
    CHECK(f.mac[0] == (uint8_t)(8 * 1 + 1) && f.n_mac() == 3 && f.n_ctr() == 3 && f.src[32] == 16 && f.src[33] == -1);
    // AAD of 14 bytes fills one block with its two length bytes, 15 bytes need two
    CHECK(tae::ccm_format(nonce, 13, 8, aad, 14, 0, f) == tae::CCM_FMT_OK);
    CHECK(f.n_mac() == 2 && f.n_ctr() == 1 && (f.mac[0] & 64) && f.mac[17] == 14 && f.mac[31] == 13);
    CHECK(tae::ccm_format(nonce, 13, 8, aad, 15, 0, f) == tae::CCM_FMT_OK);
    CHECK(f.n_mac() == 3 && f.mac[32] == 14 && f.mac[33] == 0 && f.src[32] == -1);
    // an empty frame: B_0 and A_0 alone
    CHECK(tae::ccm_format(nonce, 13, 8, nullptr, 0, 0, f) == tae::CCM_FMT_OK);
    CHECK(f.n_mac() == 1 && f.n_ctr() == 1 && f.payload_len == 0);
    // refusals leave the frame empty
    CHECK(tae::ccm_format(nonce, 6, 8, nullptr, 0, 0, f) == tae::CCM_FMT_NONCE && f.mac.empty());
    CHECK(tae::ccm_format(nonce, 14, 8, nullptr, 0, 0, f) == tae::CCM_FMT_NONCE);
    for (int m : {0, 2, 3, 5, 15, 17, 18, -4}) CHECK(tae::ccm_format(nonce, 13, m, nullptr, 0, 0, f) == tae::CCM_FMT_TAG);
    std::vector<uint8_t> long_aad(0xFF00, 1);
    CHECK(tae::ccm_format(nonce, 13, 8, long_aad.data(), 0xFF00, 0, f) == tae::CCM_FMT_AAD);
    CHECK(tae::ccm_format(nonce, 13, 8, long_aad.data(), 0xFEFF, 0, f) == tae::CCM_FMT_OK);
    CHECK(f.n_mac() == 1 + (2 + 0xFEFF + 15) / 16 && f.mac[16] == 0xFE && f.mac[17] == 0xFF);
    CHECK(tae::ccm_format(nonce, 13, 8, nullptr, 0, 0x10000, f) == tae::CCM_FMT_LEN);  // L = 2
    CHECK(tae::ccm_format(nonce, 13, 8, nullptr, 0, 0xFFFF, f) == tae::CCM_FMT_OK);
    CHECK(f.n_ctr() == 1 + 4096 && f.ctr[16 * 4096 + 14] == 0x10 && f.ctr[16 * 4096 + 15] == 0x00);
    CHECK(tae::ccm_format(nonce, 12, 8, nullptr, 0, 0x10000, f) == tae::CCM_FMT_OK && f.L == 3);
}

static void check_plan(const std::vector<tae::PubBlock> &blocks, size_t want_groups) {
    tae::CtrPlanMulti plan;
    tae::pub_plan(blocks.data(), blocks.size(), plan);
    const size_t n = blocks.size();
    CHECK(plan.map.size() == n * 16 && plan.block_slot.size() == n && plan.block_out.size() == n &&
          plan.block_len.size() == n && plan.group_slot.size() == plan.groups.size());
    CHECK(plan.groups.size() == want_groups);
    std::set<std::tuple<int32_t, int, int>> uniq, want;
    for (size_t g = 0; g < plan.groups.size(); g++)
        uniq.insert(std::make_tuple(plan.group_slot[g], plan.groups[g] >> 8, plan.groups[g] & 0xff));
    CHECK(uniq.size() == plan.groups.size());  // pairwise distinct
    for (size_t i = 0; i < n; i++) {
        CHECK(plan.block_slot[i] == blocks[i].slot && plan.block_out[i] == blocks[i].out_byte &&
              plan.block_len[i] == blocks[i].len);
        for (int pos = 0; pos < 16; pos++) {
            const int32_t g = plan.map[i * 16 + pos];
            CHECK(g >= 0 && (size_t)g < plan.groups.size());
            if (g < 0 || (size_t)g >= plan.groups.size()) continue;
            CHECK(plan.group_slot[g] == blocks[i].slot &&
                  plan.groups[g] == (uint16_t)((pos << 8) | blocks[i].bytes[pos]));
            want.insert(std::make_tuple(blocks[i].slot, pos, (int)blocks[i].bytes[pos]));
        }
    }
    CHECK(want == uniq);  // no group that no block uses
}

static void test_pub_plan() {
    const uint8_t nonce[13] = {0x00, 0x00, 0x00, 0x03, 0x02, 0x01, 0x00, 0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5};
    const uint8_t aad[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    tae::CcmFrame f;
    tae::ccm_format(nonce, 13, 8, aad, 8, 23, f);
    auto block = [](int32_t slot, const uint8_t *bytes, int64_t out, int32_t len) {
        tae::PubBlock b;
        b.slot = slot;
        std::memcpy(b.bytes, bytes, 16);
        b.out_byte = out;
        b.len = len;
        return b;
    };
    // A_0, A_1, A_2: flags and nonce give 14 groups, the counter's low byte three more; B_0 differs in the flags and
    // in the last byte (0x17)
    std::vector<tae::PubBlock> blocks = {block(0, &f.ctr[0], 0, 0), block(0, &f.ctr[16], 0, 16), block(0, &f.ctr[32], 16, 7)};
    check_plan(blocks, 14 + 1 + 3);
    blocks.push_back(block(0, &f.mac[0], 0, 0));
    check_plan(blocks, 18 + 2);
    // the same blocks under another slot share nothing
    for (int i = 0; i < 4; i++) blocks.push_back(block(3, blocks[i].bytes, 0, 16));
    check_plan(blocks, 40);
    check_plan({}, 0);
    // on iv || be64(counter) blocks: ctr_plan_multi's plan, array for array
    const uint8_t iv[8] = {0xbd, 0xd2, 0x19, 0xb8, 0xa0, 0x8d, 0xed, 0x1a};
    std::vector<tae::CtrBlock> cb;
    std::vector<tae::PubBlock> pb;
    for (int s = 0; s < 2; s++)
        for (uint64_t i = 0; i < 20; i++) {
            tae::CtrBlock c;
            c.slot = s;
            std::memcpy(c.iv, iv, 8);
            c.counter = 250 + i;
            c.out_byte = (int64_t)(16 * cb.size());
            c.len = 16;
            cb.push_back(c);
            uint8_t bytes[16];
            for (int pos = 0; pos < 16; pos++) bytes[pos] = tae::ctr_block_byte(c.iv, c.counter, pos);
            pb.push_back(block(s, bytes, c.out_byte, c.len));
        }
    tae::CtrPlanMulti a, b;
    tae::ctr_plan_multi(cb.data(), cb.size(), a);
    tae::pub_plan(pb.data(), pb.size(), b);
    CHECK(a.groups == b.groups && a.group_slot == b.group_slot && a.map == b.map && a.block_slot == b.block_slot &&
          a.block_out == b.block_out && a.block_len == b.block_len);
}

static void test_words() {
    const int L = 5, nr = 10, n = 3, n_keys = 2, M = 6;
    const size_t stride = (size_t)128 * (nr + 1) * L, n_plain = 40;
    std::vector<uint64_t> x((size_t)n * 128 * L), s0(x.size()), plain(n_plain * 8 * L), rk(n_keys * stride);
    for (auto *v : {&x, &s0, &plain, &rk})
        for (uint64_t &w : *v) w = rnd();
    const int32_t key_of[n] = {1, 0, 1};
    // stream 0: a whole payload block; stream 1: public bytes; stream 2: a partial last block (7 payload bytes, then
    // public zero padding)
    std::vector<int64_t> src(n * 16);
    for (int pos = 0; pos < 16; pos++) {
        src[pos] = 16 + pos;
        src[16 + pos] = tae::ccm_src_public((uint8_t)(0x80 + 7 * pos));
        src[32 + pos] = pos < 7 ? 33 + pos : tae::ccm_src_public(0);
    }
    for (size_t t = 0; t < x.size(); t++) {
        const size_t coef = t % L, ct = t / L, blk = ct / 128;
        const int pos = (int)((ct / 8) % 16), bit = (int)(ct % 8);
        const uint64_t *key = &rk[(size_t)key_of[blk] * stride];
        const size_t k = (size_t)(pos * 8 + bit) * L + coef;
        uint64_t want = x[t] + key[k];
        const int64_t s = src[blk * 16 + pos];
        if (s >= 0) {
            want += plain[((size_t)s * 8 + bit) * L + coef];
            want -= key[(size_t)128 * nr * L + k];
            want -= key[(size_t)128 * nr * L + k];
        } else if (coef == (size_t)L - 1) {
            want += (uint64_t)(((-(s + 1)) >> (7 - bit)) & 1) << 63;
        }
        CHECK(tae::ccm_absorb_word(x.data(), plain.data(), rk.data(), src.data(), t, L, key_of, stride, nr) == want);
    }
    // one key, no slots: the table is the key
    CHECK(tae::ccm_absorb_word(x.data(), plain.data(), rk.data(), src.data(), 7, L, nullptr, 0, nr) ==
          x[7] + rk[7] + plain[((size_t)16 * 8 + 1) * L + 2] - 2 * rk[(size_t)128 * nr * L + 7]);
    // the tag differences, written in the caller's order
    uint8_t tags[n * M];
    for (uint8_t &b : tags) b = (uint8_t)rnd();
    const int32_t out_of[n] = {2, 0, 1};
    std::vector<uint64_t> out((size_t)n * 8 * M * L, 0x5555);
    for (size_t t = 0; t < out.size(); t++)
        tae::ccm_tag_word(x.data(), s0.data(), rk.data(), tags, M, out_of, out.data(), t, L, key_of, stride, nr);
    for (int s = 0; s < n; s++)
        for (int i = 0; i < 8 * M; i++)
            for (int coef = 0; coef < L; coef++) {
                const uint64_t *key = &rk[(size_t)key_of[s] * stride];
                const size_t k = (size_t)i * L + coef;
                uint64_t want = x[(size_t)s * 128 * L + k] + s0[(size_t)s * 128 * L + k] - 2 * key[(size_t)128 * nr * L + k];
                if (coef == L - 1) want += (uint64_t)((tags[s * M + i / 8] >> (7 - i % 8)) & 1) << 63;
                CHECK(out[((size_t)out_of[s] * 8 * M + i) * L + coef] == want);
            }
}

int main() {
    test_format();
    test_pub_plan();
    test_words();
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
