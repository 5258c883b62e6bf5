// Host check of the XTS mask layer (csrc/aes_xts.hpp), following the data flow of the device kernel with bit values
// in place of ciphertexts (L = 1: a "ciphertext" is one word holding a bit, and an LWE sum is a sum whose parity is
// the XOR): rowsum_word over the RowPlan of xts_plan against the byte-wise alpha procedure of IEEE 1619 on random 16-byte
// values, the row weights, and the full decrypt data flow (mask, plain inverse cipher, mask) on IEEE 1619 vector 2.
// Stand-alone: built plain and with -fsanitize=address,undefined by tests/test_aes_xts.py.
#include <cstdio>
#include <cstring>

#include "../../tfhe-aes-2_amd/csrc/aes.hpp"
#include "../../tfhe-aes-2_amd/csrc/aes_inv.hpp"
#include "../../tfhe-aes-2_amd/csrc/aes_xts.hpp"

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

// IEEE 1619 5.2, byte-wise: the independent definition
static void alpha_bytes(uint8_t t[16]) {
    uint8_t carry = 0;
    for (int i = 0; i < 16; i++) {
        const uint8_t next = (uint8_t)(t[i] >> 7);
        t[i] = (uint8_t)((t[i] << 1) | carry);
        carry = next;
    }
    if (carry) t[0] ^= 0x87;
}

// bytes <-> the project's bit order (MSB first), one word per bit
static void to_bits(const uint8_t *bytes, size_t n, uint64_t *bits) {
    for (size_t i = 0; i < 8 * n; i++) bits[i] = (bytes[i >> 3] >> (7 - (i & 7))) & 1;
}
static void from_bits(const uint64_t *bits, size_t n, uint8_t *bytes) {
    std::memset(bytes, 0, n);
    for (size_t i = 0; i < 8 * n; i++) bytes[i >> 3] |= (uint8_t)((bits[i] & 1) << (7 - (i & 7)));
}

// the mask kernel on the host: nb blocks from n_units tweaks
static std::vector<uint64_t> masks_of(const std::vector<uint64_t> &tweaks, const tae::RowPlan &plan) {
    CHECK(tae::rowplan_ok(plan, tweaks.size()));
    std::vector<uint64_t> m(plan.n_rows());
    for (size_t t = 0; t < m.size(); t++) m[t] = tae::rowsum_word(tweaks.data(), plan, t, 1);
    return m;
}

// the forward and the inverse cipher byte-wise, AES-128, all ten rounds
static void encrypt_block(const uint8_t rk[176], const uint8_t in[16], uint8_t out[16]) {
    uint8_t st[16];
    for (int i = 0; i < 16; i++) st[i] = in[i] ^ rk[i];
    for (int r = 1; r <= 10; r++) {
        uint8_t t[16];
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++) t[4 * c + row] = tae::kSbox[st[4 * ((c + row) & 3) + row]];
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++) {
                uint8_t v = t[4 * c + row];
                if (r != 10)
                    v = (uint8_t)(tae::gf_mul(t[4 * c + row], 2) ^ tae::gf_mul(t[4 * c + ((row + 1) & 3)], 3) ^
                                  t[4 * c + ((row + 2) & 3)] ^ t[4 * c + ((row + 3) & 3)]);
                st[4 * c + row] = v ^ rk[16 * r + 4 * c + row];
            }
    }
    std::memcpy(out, st, 16);
}

static void decrypt_block(const uint8_t rk[176], const uint8_t in[16], uint8_t out[16]) {
    uint8_t st[16];
    for (int i = 0; i < 16; i++) st[i] = in[i] ^ rk[160 + i];
    for (int r = 9; r >= 0; r--) {
        uint8_t t[16];
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++)
                t[4 * c + row] = tae::kInvSbox[st[4 * ((c - row) & 3) + row]] ^ rk[16 * r + 4 * c + row];
        if (r)
            for (int c = 0; c < 4; c++)
                for (int row = 0; row < 4; row++)
                    st[4 * c + row] = (uint8_t)(tae::gf_mul(t[4 * c + row], 14) ^ tae::gf_mul(t[4 * c + ((row + 1) & 3)], 11) ^
                                                tae::gf_mul(t[4 * c + ((row + 2) & 3)], 13) ^
                                                tae::gf_mul(t[4 * c + ((row + 3) & 3)], 9));
        else
            std::memcpy(st, t, 16);
    }
    std::memcpy(out, st, 16);
}

int main() {
    // the bit order and the field arithmetic
    CHECK(tae::xts_ct_of_coef(0) == 7 && tae::xts_ct_of_coef(7) == 0 && tae::xts_ct_of_coef(8) == 15 &&
          tae::xts_ct_of_coef(127) == 120);
    {
        tae::Gf128 a = tae::xts_x_pow(0);
        for (uint64_t j = 0; j < 300; j++, a = tae::xts_alpha(a)) {
            const tae::Gf128 p = tae::xts_x_pow(j);
            CHECK(p.lo == a.lo && p.hi == a.hi);
        }
        const tae::Gf128 x128 = tae::xts_x_pow(128);
        CHECK(x128.lo == 0x87 && x128.hi == 0);
        const tae::Gf128 big = tae::xts_x_pow(0x123456789abcdefULL), split = tae::xts_gf_mul(tae::xts_x_pow(0x123456700000000ULL),
                                                                                             tae::xts_x_pow(0x89abcdefULL));
        CHECK(big.lo == split.lo && big.hi == split.hi);
    }
    // the row weights the noise rule rests on
    static const struct {
        uint64_t j;
        int w;
    } weights[] = {{0, 1}, {1, 2}, {2, 3}, {8, 4}, {121, 4}, {122, 5}, {126, 6}, {127, 7}, {128, 7}, {243, 7},
                   {244, 8}, {255, 9}, {256, 9}, {511, 11}, {1023, 13}, {4095, 14}, {65535, 81}};
    for (const auto &e : weights) CHECK(tae::xts_row_weight(e.j) == e.w);

    // the row sums of xts_plan against the byte-wise procedure: 3 units of random tweaks, every index under every unit
    static const uint64_t index[] = {0, 1, 7, 8, 121, 122, 127, 128, 255, 300, 4095};
    const size_t n_idx = sizeof(index) / sizeof(index[0]), n_units = 3;
    uint8_t T[n_units][16];
    uint64_t seed = 0x9e3779b97f4a7c15ULL;
    for (auto &t : T)
        for (auto &b : t) {
            seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
            b = (uint8_t)(seed >> 56);
        }
    std::vector<uint64_t> tweaks(n_units * 128);
    for (size_t u = 0; u < n_units; u++) to_bits(T[u], 16, &tweaks[u * 128]);
    std::vector<int32_t> unit_of;
    std::vector<uint64_t> block_index;
    for (size_t u = 0; u < n_units; u++)
        for (size_t i = 0; i < n_idx; i++) {
            unit_of.push_back((int32_t)((u + i) % n_units));
            block_index.push_back(index[i]);
        }
    const tae::RowPlan plan = tae::xts_plan(unit_of.data(), block_index.data(), block_index.size());
    CHECK(plan.n_lists() == n_idx * 128 && plan.max_width() == 14);  // distinct indices share a set; 4095 is the heaviest
    CHECK(plan.n_rows() == block_index.size() * 128 && plan.base_of.size() == plan.n_rows());
    size_t listed = 0;  // every distinct index is listed once, whole: the sum of its 128 row weights
    for (size_t i = 0; i < n_idx; i++) {
        std::vector<int16_t> rows[128];
        tae::xts_rows_of(index[i], rows);
        for (const auto &r : rows) listed += r.size();
    }
    CHECK(plan.src.size() == listed);
    const std::vector<uint64_t> masks = masks_of(tweaks, plan);
    for (size_t b = 0; b < block_index.size(); b++) {
        uint8_t want[16], got[16];
        std::memcpy(want, T[unit_of[b]], 16);
        for (uint64_t s = 0; s < block_index[b]; s++) alpha_bytes(want);
        from_bits(&masks[b * 128], 16, got);
        CHECK(!std::memcmp(want, got, 16));
        size_t heaviest = 0;
        for (int o = 0; o < 128; o++) heaviest = masks[b * 128 + o] > heaviest ? masks[b * 128 + o] : heaviest;
        CHECK((int)heaviest <= tae::xts_row_weight(block_index[b]));  // a sum of bits never exceeds its row weight
    }

    // IEEE 1619 vector 2 through the decrypt data flow: T, the masks of blocks 0 and 1, C + M, Dec, + M
    uint8_t key1[16], key2[16], tweak[16] = {0x33, 0x33, 0x33, 0x33, 0x33}, rk1[176], rk2[176], t_enc[16];
    std::memset(key1, 0x11, 16);
    std::memset(key2, 0x22, 16);
    static const uint8_t ct[32] = {0xc4, 0x54, 0x18, 0x5e, 0x6a, 0x16, 0x93, 0x6e, 0x39, 0x33, 0x40, 0x38, 0xac, 0xef, 0x83, 0x8b,
                                   0xfb, 0x18, 0x6f, 0xff, 0x74, 0x80, 0xad, 0xc4, 0x28, 0x93, 0x82, 0xec, 0xd6, 0xd3, 0x94, 0xf0};
    tae::plain_key_schedule(key1, rk1);
    tae::plain_key_schedule(key2, rk2);
    encrypt_block(rk2, tweak, t_enc);
    std::vector<uint64_t> t_bits(128);
    to_bits(t_enc, 16, t_bits.data());
    const uint64_t two[2] = {0, 1};
    const tae::RowPlan p2 = tae::xts_plan(nullptr, two, 2);
    CHECK(p2.max_width() == 2 && p2.n_lists() == 2 * 128 && p2.base_of[128] == 0 && p2.list_of[128] == 128);
    const std::vector<uint64_t> m2 = masks_of(t_bits, p2);
    for (int b = 0; b < 2; b++) {
        uint8_t m[16], x[16], y[16];
        from_bits(&m2[b * 128], 16, m);
        for (int i = 0; i < 16; i++) x[i] = ct[16 * b + i] ^ m[i];
        decrypt_block(rk1, x, y);
        for (int i = 0; i < 16; i++) CHECK((y[i] ^ m[i]) == 0x44);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
