// Host check of the counter-mode round-1 plan (csrc/ctr_plan.hpp): every (block, position) maps to the group
// holding that block's byte, groups are unique and ordered (iv positions first, then positions 8..15 with
// their values in first-appearance order), and a wrapping range is refused.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../../tfhe-aes-2_amd/csrc/ctr_plan.hpp"

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

static void check_range(const uint8_t iv[8], uint64_t first, size_t n, size_t want_groups) {
    tae::CtrPlan plan;
    CHECK(tae::ctr_plan(iv, first, n, plan));
    CHECK(plan.groups.size() == want_groups);
    CHECK(plan.map.size() == n * 16);
    std::set<uint16_t> uniq(plan.groups.begin(), plan.groups.end());
    CHECK(uniq.size() == plan.groups.size());
    for (size_t g = 0; g < plan.groups.size() && g < 8; g++) CHECK(plan.groups[g] == ((g << 8) | iv[g]));
    for (size_t g = 1; g < plan.groups.size(); g++) CHECK((plan.groups[g] >> 8) >= (plan.groups[g - 1] >> 8));
    int32_t high = -1;  // first appearance: scanning blocks per position, a new group index is the next one
    for (int pos = 0; pos < 16; pos++)
        for (size_t i = 0; i < n; i++) {
            const uint64_t ctr = first + i;
            uint8_t blk[16];
            for (int p = 0; p < 8; p++) blk[p] = iv[p];
            for (int p = 8; p < 16; p++) blk[p] = (uint8_t)(ctr >> (8 * (15 - p)));
            const int32_t g = plan.map[i * 16 + pos];
            CHECK(g >= 0 && (size_t)g < plan.groups.size());
            CHECK(plan.groups[g] == (uint16_t)((pos << 8) | blk[pos]));
            CHECK(g <= high + 1);
            if (g > high) high = g;
        }
    CHECK(n == 0 || (size_t)high + 1 == plan.groups.size());
}

int main() {
    const uint8_t iv[8] = {0xbd, 0xd2, 0x19, 0xb8, 0xa0, 0x8d, 0xed, 0x1a};
    check_range(iv, 1, 128, 143);
    check_range(iv, 1, 1024, 275);
    check_range(iv, 0xFE, 3, 19);
    check_range(iv, 897, 128, 144);
    check_range(iv, 1, 1, 16);
    check_range(iv, 0, 0, 0);
    check_range(iv, 0xFFFFFFFFFFFFFF00ull, 256, 8 + 7 + 256);  // up to the last counter, no wrap
    const uint8_t same[8] = {7, 7, 7, 7, 7, 7, 7, 7};          // equal iv bytes are still one group per position
    check_range(same, 0x0707070707070707ull, 1, 16);
    tae::CtrPlan plan;
    plan.groups.assign(3, 1);
    CHECK(!tae::ctr_plan(iv, UINT64_MAX, 2, plan));
    CHECK(plan.groups.size() == 3);  // untouched
    CHECK(tae::ctr_plan(iv, UINT64_MAX, 1, plan) && plan.groups.size() == 16);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
