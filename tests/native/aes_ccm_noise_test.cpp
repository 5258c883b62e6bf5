// The host model's CCM noise bookkeeping (model.cpp aes_ccm_noise_schedule) called in the product library, no GPU
// call: the squared levels of DESIGN.md 5.13 (plaintext bit 8 + 1, round 0 of a chain step 8 + 1 + 1 at a public
// byte and 8 + 8 + 1 at a payload byte, tag-difference bit 16), the ids the output bits carry, the legal XORs, and
// rounds = 1 refused.  Built and run by tests/test_aes_ccm.py (CPU only).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/aes_ccm.hpp"

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
struct CcmNoise {
    std::vector<NoiseLevel> plain, tag_diff;
    std::vector<std::vector<uint64_t>> step_round0;
};
CcmNoise aes_ccm_noise_schedule(const std::vector<NoiseLevel> &rk, const CcmFrame &frame, int rounds,
                                uint64_t max_noise_sq, int nr);
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

static int code_of(const std::vector<tae::NoiseLevel> &rk, const tae::CcmFrame &f, int rounds, uint64_t max, int nr) {
    try {
        tae::aes_ccm_noise_schedule(rk, f, rounds, max, nr);
    } catch (const tae::ModelError &e) {
        return e.code;
    }
    return 0;
}

int main() {
    const uint64_t max = 64;  // params_sqrd_lvl_64
    const int E_NOISE = 1, E_PARAM = 3;
    const uint8_t nonce[13] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13};
    const uint8_t aad[8] = {};
    tae::CcmFrame f;
    CHECK(tae::ccm_format(nonce, 13, 8, aad, 8, 23, f) == tae::CCM_FMT_OK);  // B_0, one AAD block, 16 + 7 payload bytes
    for (int nr : {10, 14}) {
        const std::vector<tae::NoiseLevel> rk = fresh((size_t)128 * (nr + 1));
        const tae::CcmNoise out = tae::aes_ccm_noise_schedule(rk, f, nr, max, nr);
        CHECK(out.plain.size() == 23 * 8 && out.tag_diff.size() == 64 && out.step_round0.size() == 3);
        for (size_t i = 0; i < out.plain.size(); i++) {
            // one circuit-bootstrap output and the last round key's bit at the byte's place in its block
            CHECK(out.plain[i].noise_level_squared == 9 && out.plain[i].components.size() == 2);
            CHECK(has(out.plain[i], rk[(size_t)128 * nr + i % 128].components[0]));
        }
        for (int i = 0; i < 128; i++) {
            CHECK(out.step_round0[0][i] == 8 + 1 + 1);                  // the AAD block: public
            CHECK(out.step_round0[1][i] == 8 + 8 + 1);                  // a whole payload block
            CHECK(out.step_round0[2][i] == (i < 56 ? 8 + 8 + 1 : 10));  // 7 payload bytes, then the padding
        }
        for (int i = 0; i < 64; i++) {
            // X'_last + S'_0: two circuit-bootstrap outputs and no key bit
            CHECK(out.tag_diff[i].noise_level_squared == 16 && out.tag_diff[i].components.size() == 2);
            for (const tae::NoiseLevel &k : rk) CHECK(!has(out.tag_diff[i], k.components[0]));
        }
        // two tag-difference bits of a frame, and one with a plaintext bit of another position
        tae::NoiseLevel v = out.tag_diff[0];
        v.add_assign(out.tag_diff[1], max);
        v.add_assign(out.plain[9], max);
        CHECK(v.noise_level_squared == 16 + 16 + 9);
        // the ids are fresh per call
        const tae::CcmNoise again = tae::aes_ccm_noise_schedule(rk, f, nr, max, nr);
        CHECK(again.tag_diff[0].components != out.tag_diff[0].components);
        CHECK(code_of(rk, f, 2, max, nr) == 0);
        CHECK(code_of(rk, f, 1, max, nr) == E_PARAM);
        CHECK(code_of(rk, f, nr + 1, max, nr) == E_PARAM);
        // the cap is enforced: 32 is below a middle round's 33
        CHECK(code_of(rk, f, nr, 32, nr) == E_NOISE);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
