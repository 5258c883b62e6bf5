// The AEAD open's host layer (csrc/aead_open.hpp) stand-alone, on plain bit values: the verdict plan's groups, padding
// and indices, the gate plan's frame_of_byte and pass indices, the three truth tables, and both plans run end to end:
// an authentic frame keeps its payload with ok = 1; a single 1 at difference bit 0, at the last bit or next to a padded
// group gives ok = 0 and an all-zero payload.  Built and run by tests/test_aead_open.py, plain and sanitized.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/aead_open.hpp"

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                \
        }                                                           \
    } while (0)

using namespace tae;

static std::vector<uint8_t> payload_bits(size_t n_bytes) {
    std::vector<uint8_t> v(n_bytes * 8);
    for (size_t g = 0; g < n_bytes; g++) {
        const unsigned byte = (unsigned)(0xA7 + 37 * g) & 0xFF;
        for (int b = 0; b < 8; b++) v[g * 8 + b] = (uint8_t)((byte >> (7 - b)) & 1);
    }
    return v;
}

int main() {
    // ---- the tag lengths ----
    for (int t = -1; t <= 20; t++) {
        const bool want = t == 4 || t == 6 || t == 8 || t == 10 || (t >= 12 && t <= 16);
        CHECK(aead_tag_len_ok(t) == want);
    }
    // ---- the tables ----
    const AeadOpenTables tab = aead_open_tables();
    CHECK(tab.or8.size() == 256 && tab.nor8.size() == 256 && tab.gate.size() == 512);
    for (unsigned v = 0; v < 256; v++) {
        CHECK(tab.or8[v] == (v ? 1u : 0u) && tab.nor8[v] == (v ? 0u : 1u));
        CHECK(tab.gate[2 * v + 1] == v && tab.gate[2 * v] == 0);
    }
    // ---- the verdict plan: groups, padding, indices ----
    struct Want {
        int tag_len;
        std::vector<size_t> groups;
    };
    const Want wants[] = {{4, {4, 1}},      {6, {6, 1}},      {8, {8, 1}},      {10, {10, 2, 1}}, {12, {12, 2, 1}},
                          {13, {13, 2, 1}}, {14, {14, 2, 1}}, {15, {15, 2, 1}}, {16, {16, 2, 1}}};
    for (const Want &w : wants)
        for (size_t n : {(size_t)1, (size_t)3}) {
            const VerdictPlan p = aead_verdict_plan(w.tag_len, n);
            CHECK(p.groups == w.groups && p.levels() == (int)w.groups.size() && p.n_frames == n);
            CHECK(p.bits[0] == 8 * (size_t)w.tag_len);
            for (int l = 0; l < p.levels(); l++) {
                if (l) CHECK(p.bits[l] == p.groups[l - 1]);
                CHECK(p.idx[l].size() == n * p.groups[l] * 8);
                for (size_t f = 0; f < n; f++)
                    for (size_t s = 0; s < p.groups[l] * 8; s++) {
                        const int32_t got = p.idx[l][f * p.groups[l] * 8 + s];
                        // in order; the tail of the last group is the zero ciphertext
                        CHECK(got == (s < p.bits[l] ? (int32_t)(f * p.bits[l] + s) : -1));
                    }
            }
        }
    {  // 13 bytes: level 1 has 13 bits in 2 groups (3 pads), level 2 has 2 bits in 1 group (6 pads)
        const VerdictPlan p = aead_verdict_plan(13, 2);
        size_t pads1 = 0, pads2 = 0;
        for (int32_t s : p.idx[1]) pads1 += s < 0;
        for (int32_t s : p.idx[2]) pads2 += s < 0;
        CHECK(pads1 == 2 * 3 && pads2 == 2 * 6);
        CHECK(p.idx[1][13] == -1 && p.idx[1][12] == 12 && p.idx[1][16] == 13 && p.idx[2][8] == 2 && p.idx[2][10] == -1);
    }
    // ---- the gate plan ----
    {
        const size_t lens[] = {17, 0, 3};
        const GatePlan g = aead_gate_plan(lens, 3);
        CHECK(g.n_bytes() == 20 && g.n_frames == 3);
        for (size_t i = 0; i < 20; i++) CHECK(g.frame_of_byte[i] == (i < 17 ? 0 : 2));
        const std::vector<int32_t> ix = aead_gate_pass_index(g, 14, 6);  // the second pass of 14: the frame changes inside
        CHECK(ix.size() == 6 * 9);
        for (size_t k = 0; k < 6; k++) {
            for (int b = 0; b < 8; b++) CHECK(ix[k * 9 + b] == (int32_t)(3 + k * 8 + b));
            CHECK(ix[k * 9 + 8] == (k < 3 ? 0 : 2));
        }
        const size_t none[] = {0};
        CHECK(aead_gate_plan(none, 1).n_bytes() == 0);
        const size_t one[] = {1};
        CHECK(aead_gate_plan(one, 1).frame_of_byte == std::vector<int32_t>{0});
    }
    // ---- both plans on plain bits ----
    for (int tag_len : {4, 8, 13, 16}) {
        const size_t bits = 8 * (size_t)tag_len;
        // frames: authentic; bit 0; the last bit; the last bit of the first level-1 group; the first bit of the last,
        // padded level-1 group (tag_len 13: difference bits 96 .. 103)
        std::vector<size_t> ones = {bits /* none */, 0, bits - 1, 63 % bits, bits - 8};
        const size_t n = ones.size();
        const size_t lens[] = {17, 0, 3, 5, 1};
        std::vector<uint8_t> diff(n * bits, 0);
        for (size_t f = 0; f < n; f++)
            if (ones[f] < bits) diff[f * bits + ones[f]] = 1;
        const VerdictPlan vp = aead_verdict_plan(tag_len, n);
        const std::vector<uint8_t> ok = aead_verdict_plain(vp, diff);
        CHECK(ok.size() == n && ok[0] == 1);
        for (size_t f = 1; f < n; f++) CHECK(ok[f] == 0);
        const GatePlan gp = aead_gate_plan(lens, n);
        const std::vector<uint8_t> plain = payload_bits(gp.n_bytes());
        for (size_t pass : {(size_t)14, (size_t)1, (size_t)1000}) {
            const std::vector<uint8_t> out = aead_gate_plain(gp, plain, ok, pass);
            CHECK(out.size() == plain.size());
            for (size_t g = 0; g < gp.n_bytes(); g++)
                for (int b = 0; b < 8; b++) CHECK(out[g * 8 + b] == (gp.frame_of_byte[g] == 0 ? plain[g * 8 + b] : 0));
        }
        // every single difference bit alone flips the verdict
        for (size_t i = 0; i < bits; i++) {
            std::vector<uint8_t> d(bits, 0);
            d[i] = 1;
            CHECK(aead_verdict_plain(aead_verdict_plan(tag_len, 1), d)[0] == 0);
        }
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
