// The host model's GCM noise bookkeeping (model.cpp aes_ghash_key_noise_schedule, aes_gcm_noise_schedule) called in
// the product library, no GPU call: the levels of DESIGN.md 5.14 (a partial chunk at most 56, a reduced bit at most
// 34, a square's row at most 5, table bits at 1 with distinct ids, payload bits at 8 + 1, a tag-difference bit at its
// chunk count), the legal XORs and the refusals.  Built and run by tests/test_aes_gcm.py (CPU only).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/aes_gcm.hpp"

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
struct GhashKeyNoise {
    std::vector<NoiseLevel> table;
    uint64_t max_chunk = 0, max_reduced = 0, max_square = 0;
};
GhashKeyNoise aes_ghash_key_noise_schedule(const std::vector<NoiseLevel> &rk, int n_powers, int rounds,
                                           uint64_t max_noise_sq, int nr);
struct GcmNoise {
    std::vector<NoiseLevel> plain, tag_diff;
    uint64_t max_chunk = 0;
};
GcmNoise aes_gcm_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &hk, const GcmFrame &frame,
                                int rounds, uint64_t max_noise_sq, int nr);
}  // namespace tae

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                \
        }                                                           \
    } while (0)

static std::vector<tae::NoiseLevel> fresh(size_t n) {
    std::vector<tae::NoiseLevel> v(n);
    for (auto &x : v) x = {1, {tae::next_ct_id()}};
    return v;
}

static bool has(const tae::NoiseLevel &x, uint64_t id) {
    return std::binary_search(x.components.begin(), x.components.end(), id);
}

template <class F>
static int code_of(F fn) {
    try {
        fn();
    } catch (const tae::ModelError &e) {
        return e.code;
    }
    return 0;
}

static tae::GcmFrame frame(size_t aad_len, size_t data_len, int tag_len) {
    const uint8_t iv[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    const std::vector<uint8_t> aad(aad_len, 0xA5), data(data_len, 0x5A);
    tae::GcmFrame f;
    CHECK(tae::gcm_format(iv, 12, aad.data(), aad_len, data.data(), data_len, tag_len, f) == tae::GCM_FMT_OK);
    return f;
}

int main() {
    const uint64_t max = 64;  // params_sqrd_lvl_64
    const int E_NOISE = 1, E_PARAM = 3;
    for (int nr : {10, 14}) {
        const std::vector<tae::NoiseLevel> rk = fresh((size_t)128 * (nr + 1));
        // ---- the power table: identity, square, product, square of a square, product of a square ----
        const tae::GhashKeyNoise hk = tae::aes_ghash_key_noise_schedule(rk, 5, nr, max, nr);
        CHECK(hk.table.size() == 5 * 128);
        CHECK(hk.max_chunk == 56 && hk.max_reduced <= 34 && hk.max_reduced > 8 && hk.max_square <= 5 && hk.max_square >= 2);
        std::set<uint64_t> ids;
        for (const tae::NoiseLevel &x : hk.table) {
            CHECK(x.noise_level_squared == 1 && x.components.size() == 1);
            ids.insert(x.components[0]);
            for (const tae::NoiseLevel &k : rk) CHECK(k.components[0] != x.components[0]);
        }
        CHECK(ids.size() == hk.table.size());
        // the cap is enforced: a chunk of 7 partial bits is 56; without a product nothing passes the cipher's 33
        CHECK(code_of([&] { tae::aes_ghash_key_noise_schedule(rk, 3, nr, 55, nr); }) == E_NOISE);
        CHECK(code_of([&] { tae::aes_ghash_key_noise_schedule(rk, 2, nr, 55, nr); }) == 0);
        CHECK(code_of([&] { tae::aes_ghash_key_noise_schedule(rk, 0, nr, max, nr); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_ghash_key_noise_schedule(rk, 65, nr, max, nr); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_ghash_key_noise_schedule(rk, 2, nr + 1, max, nr); }) == E_PARAM);

        // ---- a frame: 8 bytes of AAD, 17 of payload, m = 4 ----
        const tae::GcmFrame f = frame(8, 17, 12);
        const std::vector<tae::NoiseLevel> table4(hk.table.begin(), hk.table.begin() + 4 * 128);
        const tae::GcmNoise out = tae::aes_gcm_noise_schedule(rk, table4, f, nr, max, nr);
        CHECK(out.plain.size() == 17 * 8 && out.tag_diff.size() == 96 && out.max_chunk == 64);
        for (size_t i = 0; i < out.plain.size(); i++) {
            CHECK(out.plain[i].noise_level_squared == 9 && out.plain[i].components.size() == 2);
            CHECK(has(out.plain[i], rk[(size_t)128 * nr + i % 128].components[0]));
        }
        std::vector<std::vector<int32_t>> rows;
        tae::gcm_frame_rows(f, rows);
        for (size_t r = 0; r < out.tag_diff.size(); r++) {
            // the sum of the row's refreshed chunks: fresh ids, no key bit, no table bit
            const size_t chunks = tae::gcm_row_chunks(rows[r].size());
            CHECK(chunks >= 2 && out.tag_diff[r].noise_level_squared == chunks && out.tag_diff[r].components.size() == chunks);
            for (const tae::NoiseLevel &k : rk) CHECK(!has(out.tag_diff[r], k.components[0]));
            for (const tae::NoiseLevel &h : table4) CHECK(!has(out.tag_diff[r], h.components[0]));
        }
        // two tag-difference bits of a frame, and one with a payload bit
        tae::NoiseLevel v = out.tag_diff[0];
        v.add_assign(out.tag_diff[1], max);
        v.add_assign(out.plain[9], max);
        CHECK(v.noise_level_squared == out.tag_diff[0].noise_level_squared + out.tag_diff[1].noise_level_squared + 9);
        // the empty frame: every row its E(J0) bit alone, one chunk, level 1
        const tae::GcmNoise none = tae::aes_gcm_noise_schedule(rk, table4, frame(0, 0, 16), nr, max, nr);
        CHECK(none.plain.empty() && none.tag_diff.size() == 128 && none.max_chunk == 9);
        for (const tae::NoiseLevel &x : none.tag_diff) CHECK(x.noise_level_squared == 1);
        // refusals: m = 5 against 4 powers, one round, a chunk cap below 9 + 55
        CHECK(code_of([&] { tae::aes_gcm_noise_schedule(rk, table4, frame(16, 33, 16), nr, max, nr); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_gcm_noise_schedule(rk, table4, f, 1, max, nr); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_gcm_noise_schedule(rk, table4, f, nr, 63, nr); }) == E_NOISE);
    }
    // an over-long frame: 100 dense hashed blocks, about 6400 sources and 100 chunks a row
    {
        const std::vector<tae::NoiseLevel> rk = fresh((size_t)128 * 11), big = fresh((size_t)128 * 128);
        const tae::GcmFrame f = frame(0, 99 * 16, 16);
        std::vector<std::vector<int32_t>> rows;
        tae::gcm_frame_rows(f, rows);
        size_t most = 0;
        for (const auto &r : rows) most = std::max(most, tae::gcm_row_chunks(r.size()));
        CHECK(most > 64 && tae::gcm_frame_check(f, 128, rows) == tae::GCM_PLAN_NOISE);
        CHECK(code_of([&] { tae::aes_gcm_noise_schedule(rk, big, f, 10, max, 10); }) == E_NOISE);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
