// The host model's XTS noise bookkeeping (model.cpp aes_xts_tweak_noise_schedule / aes_xts_noise_schedule) called in
// the product library, no GPU call: an output bit of block j is 8 + 1 + its row weight (9 + w(j) at the heaviest
// row) and carries the ids of the tweak bits in its row, for j in {0, 31, 127}; two outputs that share a tweak bit
// cannot be added, outputs of different tweaks can.  Built and run by tests/test_aes_xts.py (CPU only).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/aes_xts.hpp"

namespace tae {
// model.hpp's declarations (the header itself needs the HIP runtime's)
struct ModelError {
    int code;
    std::string msg;
};
struct NoiseLevel {
    uint64_t noise_level_squared = 0;
    std::vector<uint64_t> components;
    void add_assign(const NoiseLevel &rhs, uint64_t max_noise_sq);
};
uint64_t next_ct_id();
std::vector<NoiseLevel> aes_xts_tweak_noise_schedule(const std::vector<NoiseLevel> &rk2, int rounds, uint64_t max_noise_sq,
                                                     int nr);
std::vector<NoiseLevel> aes_xts_noise_schedule(const std::vector<NoiseLevel> &dk1, const std::vector<NoiseLevel> &tweak,
                                               uint64_t j, int rounds, uint64_t max_noise_sq, int nr);
}  // namespace tae

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

static std::vector<tae::NoiseLevel> fresh(size_t n) {
    std::vector<tae::NoiseLevel> v(n);
    for (auto &x : v) x = {1, {tae::next_ct_id()}};
    return v;
}

static bool has(const tae::NoiseLevel &x, uint64_t id) {
    return std::binary_search(x.components.begin(), x.components.end(), id);
}

int main() {
    const uint64_t max = 64;  // params_sqrd_lvl_64
    const int E_NOISE = 1, E_INDEP = 2;
    const std::vector<tae::NoiseLevel> dk1 = fresh(44 * 32), rk2 = fresh(44 * 32);
    const std::vector<tae::NoiseLevel> t_a = tae::aes_xts_tweak_noise_schedule(rk2, 10, max, 10);
    const std::vector<tae::NoiseLevel> t_b = tae::aes_xts_tweak_noise_schedule(rk2, 10, max, 10);
    CHECK(t_a.size() == 128);
    for (int i = 0; i < 128; i++) {
        CHECK(t_a[i].noise_level_squared == 1 && t_a[i].components.size() == 1);
        CHECK(t_a[i].components != t_b[i].components);  // every refresh has ids of its own
    }
    static const struct {
        uint64_t j;
        uint64_t w;
    } cases[] = {{0, 1}, {31, 4}, {127, 7}};
    for (const auto &c : cases) {
        const std::vector<tae::NoiseLevel> out = tae::aes_xts_noise_schedule(dk1, t_a, c.j, 10, max, 10);
        std::vector<int16_t> rows[128];
        tae::xts_rows_of(c.j, rows);
        uint64_t top = 0;
        for (int o = 0; o < 128; o++) {
            CHECK(out[o].noise_level_squared == 9 + rows[o].size());
            top = std::max(top, out[o].noise_level_squared);
            // one circuit-bootstrap output, one key bit, the tweak bits of the row
            CHECK(out[o].components.size() == 2 + rows[o].size());
            for (int16_t src : rows[o]) CHECK(has(out[o], t_a[src].components[0]));
            CHECK(has(out[o], dk1[o].components[0]));  // round key 0 of the decryption key: words 0..3
        }
        CHECK(top == 9 + c.w);
    }
    // block 0 bit 15 and block 1 bit 14 of one unit share tweak bit 15; under another tweak they share nothing
    const std::vector<tae::NoiseLevel> b0 = tae::aes_xts_noise_schedule(dk1, t_a, 0, 10, max, 10);
    const std::vector<tae::NoiseLevel> b1 = tae::aes_xts_noise_schedule(dk1, t_a, 1, 10, max, 10);
    const std::vector<tae::NoiseLevel> other = tae::aes_xts_noise_schedule(dk1, t_b, 1, 10, max, 10);
    int code = 0;
    try {
        tae::NoiseLevel x = b0[15];
        x.add_assign(b1[14], max);
    } catch (const tae::ModelError &e) {
        code = e.code;
    }
    CHECK(code == E_INDEP);
    tae::NoiseLevel y = b0[15];
    y.add_assign(other[14], max);
    CHECK(y.noise_level_squared == b0[15].noise_level_squared + other[14].noise_level_squared);
    // the cap: 9 + w(j) <= 64
    code = 0;
    try {
        tae::aes_xts_noise_schedule(dk1, t_a, 65535, 10, max, 10);
    } catch (const tae::ModelError &e) {
        code = e.code;
    }
    CHECK(code == E_NOISE);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
