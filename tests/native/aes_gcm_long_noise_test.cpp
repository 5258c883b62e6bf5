// The host model's bookkeeping of segmented GHASH (model.cpp aes_ghash_stride_key_noise_schedule,
// aes_gcm_long_noise_schedule) called in the product library, no GPU call: the levels of DESIGN.md 5.16 (an inner
// chunk at most 64, an inner row its chunk count, a product as the key schedule replays it, the first final chunk
// 9 + at most 55, a tag-difference bit at its chunk count with fresh ids and no key bit, payload bits at 8 + 1), the
// stride key's ids, the legal XORs and the refusals.  Built and run by tests/test_aes_gcm_long.py (CPU only).
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
GhashKeyNoise aes_ghash_stride_key_noise_schedule(const std::vector<NoiseLevel> &hk, size_t seg, int n_strides,
                                                  uint64_t max_noise_sq);
struct GcmNoise {
    std::vector<NoiseLevel> plain, tag_diff;
    uint64_t max_chunk = 0;
};
GcmNoise aes_gcm_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &hk, const GcmFrame &frame,
                                int rounds, uint64_t max_noise_sq, int nr);
struct GcmLongNoise {
    std::vector<NoiseLevel> plain, tag_diff;
    uint64_t max_inner_chunk = 0, max_inner_row = 0, max_part_chunk = 0, max_reduced = 0, max_chunk = 0;
};
GcmLongNoise aes_gcm_long_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &hk,
                                         const std::vector<NoiseLevel> &sk, size_t seg, const GcmFrame &frame, int rounds,
                                         uint64_t max_noise_sq, int nr);
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

static tae::GcmFrame frame(size_t aad_len, size_t data_len, int tag_len, uint8_t fill = 0x5A) {
    const uint8_t iv[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    const std::vector<uint8_t> aad(aad_len, 0xA5), data(data_len, fill);
    tae::GcmFrame f;
    CHECK(tae::gcm_format(iv, 12, aad.data(), aad_len, data.data(), data_len, tag_len, f) == tae::GCM_FMT_OK);
    return f;
}

int main() {
    const uint64_t max = 64;  // params_sqrd_lvl_64
    const int E_NOISE = 1, E_PARAM = 3;
    for (int nr : {10, 14}) {
        const std::vector<tae::NoiseLevel> rk = fresh((size_t)128 * (nr + 1));
        const tae::GhashKeyNoise hk = tae::aes_ghash_key_noise_schedule(rk, 4, nr, max, nr);
        // ---- the stride key: seg = 2, strides 1 .. 5 (a copy, a square, a product, a square, a product) ----
        const tae::GhashKeyNoise sk = tae::aes_ghash_stride_key_noise_schedule(hk.table, 2, 5, max);
        CHECK(sk.table.size() == 5 * 128 && sk.max_chunk == 56 && sk.max_reduced <= 34 && sk.max_square <= 5 && sk.max_square >= 2);
        std::set<uint64_t> ids;
        for (size_t i = 0; i < sk.table.size(); i++) {
            const tae::NoiseLevel &x = sk.table[i];
            CHECK(x.noise_level_squared == 1 && x.components.size() == 1);
            ids.insert(x.components[0]);
            // entry 0 is the table's block seg - 1, ids included; nothing later shares an id with the table
            if (i < 128) CHECK(x.components[0] == hk.table[128 + i].components[0]);
            else
                for (const tae::NoiseLevel &h : hk.table) CHECK(h.components[0] != x.components[0]);
        }
        CHECK(ids.size() == sk.table.size());
        CHECK(code_of([&] { tae::aes_ghash_stride_key_noise_schedule(hk.table, 0, 2, max); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_ghash_stride_key_noise_schedule(hk.table, 5, 2, max); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_ghash_stride_key_noise_schedule(hk.table, 2, 0, max); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_ghash_stride_key_noise_schedule(hk.table, 2, 65, max); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_ghash_stride_key_noise_schedule(hk.table, 2, 3, 55); }) == E_NOISE);  // a product's chunk is 56
        CHECK(code_of([&] { tae::aes_ghash_stride_key_noise_schedule(hk.table, 2, 2, 55); }) == 0);

        // ---- a frame: 8 bytes of AAD, 40 of payload, m = 5; seg = 2: C = 3, the top segment holds one block ----
        const tae::GcmFrame f = frame(8, 40, 12);
        const tae::GcmLongNoise out = tae::aes_gcm_long_noise_schedule(rk, hk.table, sk.table, 2, f, nr, max, nr);
        CHECK(out.plain.size() == 40 * 8 && out.tag_diff.size() == 96);
        CHECK(out.max_inner_chunk == 64 && out.max_inner_row >= 2 && out.max_inner_row <= 4);  // at most 256 sources
        CHECK(out.max_part_chunk == 56 && out.max_reduced <= 34 && out.max_reduced > 8 && out.max_chunk == 64);
        for (size_t i = 0; i < out.plain.size(); i++) {
            CHECK(out.plain[i].noise_level_squared == 9 && out.plain[i].components.size() == 2);
            CHECK(has(out.plain[i], rk[(size_t)128 * nr + i % 128].components[0]));
        }
        std::vector<std::vector<int32_t>> rows;
        tae::gcm_long_final_rows(f, 2, 0, rows);
        size_t most = 0;  // segment 0 holds the sparse length block and one dense block: one or two chunks a row
        for (size_t r = 0; r < out.tag_diff.size(); r++) most = std::max(most, tae::gcm_row_chunks(rows[r].size()));
        CHECK(most == 2);
        for (size_t r = 0; r < out.tag_diff.size(); r++) {
            const size_t chunks = tae::gcm_row_chunks(rows[r].size());
            CHECK(out.tag_diff[r].noise_level_squared == chunks && out.tag_diff[r].components.size() == chunks);
            for (const tae::NoiseLevel &k : rk) CHECK(!has(out.tag_diff[r], k.components[0]));
            for (const tae::NoiseLevel &h : hk.table) CHECK(!has(out.tag_diff[r], h.components[0]));
            for (const tae::NoiseLevel &s : sk.table) CHECK(!has(out.tag_diff[r], s.components[0]));
        }
        // two tag-difference bits of a frame, and one with a payload bit
        tae::NoiseLevel v = out.tag_diff[0];
        v.add_assign(out.tag_diff[1], max);
        v.add_assign(out.plain[9], max);
        CHECK(v.noise_level_squared == out.tag_diff[0].noise_level_squared + out.tag_diff[1].noise_level_squared + 9);
        // C = 1: the levels of the single-table schedule
        const tae::GcmFrame g = frame(0, 5, 16);  // m = 2
        const tae::GcmLongNoise one = tae::aes_gcm_long_noise_schedule(rk, hk.table, sk.table, 2, g, nr, max, nr);
        const tae::GcmNoise old = tae::aes_gcm_noise_schedule(rk, hk.table, g, nr, max, nr);
        CHECK(one.max_inner_chunk == 0 && one.max_part_chunk == 0 && one.max_chunk == old.max_chunk);
        CHECK(one.tag_diff.size() == old.tag_diff.size());
        for (size_t r = 0; r < one.tag_diff.size(); r++)
            CHECK(one.tag_diff[r].noise_level_squared == old.tag_diff[r].noise_level_squared);
        // refusals: shape, rounds, a chunk cap below 9 + 55, a product's chunk cap
        const std::vector<tae::NoiseLevel> sk1(sk.table.begin(), sk.table.begin() + 128);
        CHECK(code_of([&] { tae::aes_gcm_long_noise_schedule(rk, hk.table, sk.table, 0, f, nr, max, nr); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_gcm_long_noise_schedule(rk, hk.table, sk.table, 5, f, nr, max, nr); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_gcm_long_noise_schedule(rk, hk.table, sk1, 2, f, nr, max, nr); }) == E_PARAM);  // C - 1 = 2
        CHECK(code_of([&] { tae::aes_gcm_long_noise_schedule(rk, hk.table, {}, 2, g, nr, max, nr); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_gcm_long_noise_schedule(rk, hk.table, sk.table, 2, f, 1, max, nr); }) == E_PARAM);
        CHECK(code_of([&] { tae::aes_gcm_long_noise_schedule(rk, hk.table, sk.table, 2, f, nr, 63, nr); }) == E_NOISE);
    }
    // 100 hashed blocks: accepted at seg = 31 whatever the data, refused at seg = 48 for 0xA5
    {
        const std::vector<tae::NoiseLevel> rk = fresh((size_t)128 * 11), hk = fresh((size_t)128 * 48), sk = fresh((size_t)128 * 3);
        const std::vector<tae::NoiseLevel> hk31(hk.begin(), hk.begin() + 128 * 31);
        const tae::GcmFrame fa = frame(0, 99 * 16, 16, 0xA5), ff = frame(0, 99 * 16, 16, 0xFF);
        const tae::GcmLongNoise a = tae::aes_gcm_long_noise_schedule(rk, hk31, sk, 31, fa, 10, max, 10);
        CHECK(a.max_inner_chunk == 64 && a.max_inner_row <= 46 && a.max_inner_row > 30 && a.max_chunk == 64);
        size_t top = 0;
        for (const tae::NoiseLevel &x : a.tag_diff) top = std::max<size_t>(top, x.noise_level_squared);
        CHECK(top <= 46 && top > 30);
        const tae::GcmLongNoise b = tae::aes_gcm_long_noise_schedule(rk, hk31, sk, 31, ff, 10, max, 10);
        CHECK(b.max_inner_row == 62 && b.max_chunk == 64);  // 31 * 126 = 3906 sources: 62 chunks
        CHECK(code_of([&] { tae::aes_gcm_long_noise_schedule(rk, hk, sk, 48, fa, 10, max, 10); }) == E_NOISE);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
