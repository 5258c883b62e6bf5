// Host check of the generalised plain key expansion (csrc/aes_plain.cpp, FIPS-197 5.2) at Nk = 4, 6 and 8:
// expands the FIPS-197 appendix C keys, checks words of appendix A's expansions, and runs the plain cipher and
// inverse cipher over Nr = Nk + 6 rounds against C.1, C.2 and C.3.  The cipher here is byte-wise and independent
// of the library's: xtime multiplication, the S-box from the field inverse and the affine map.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/aes.hpp"

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

static uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
static uint8_t mul(uint8_t a, uint8_t b) {
    uint8_t r = 0;
    for (int i = 0; i < 8; i++, a = xtime(a))
        if ((b >> i) & 1) r ^= a;
    return r;
}
static uint8_t sbox(uint8_t x) {
    uint8_t inv = 0;
    for (int y = 1; y < 256 && x; y++)
        if (mul(x, (uint8_t)y) == 1) inv = (uint8_t)y;
    uint8_t s = 0x63;
    for (int sh = 0; sh < 5; sh++) s ^= (uint8_t)((inv << sh) | (inv >> (8 - sh)));
    return s;
}

static void hex(const char *h, uint8_t *out, int n) {
    for (int i = 0; i < n; i++) {
        unsigned v = 0;
        std::sscanf(h + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}

// state index 4 * col + row, as the library lays blocks out
static void encrypt(const uint8_t *rk, int nr, const uint8_t in[16], uint8_t out[16]) {
    uint8_t s[16], t[16];
    for (int i = 0; i < 16; i++) s[i] = in[i] ^ rk[i];
    for (int r = 1; r <= nr; r++) {
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++) t[4 * c + row] = sbox(s[4 * ((c + row) & 3) + row]);
        if (r < nr) {
            for (int c = 0; c < 4; c++)
                for (int row = 0; row < 4; row++)
                    s[4 * c + row] = (uint8_t)(mul(t[4 * c + row], 2) ^ mul(t[4 * c + ((row + 1) & 3)], 3) ^
                                               t[4 * c + ((row + 2) & 3)] ^ t[4 * c + ((row + 3) & 3)]);
        } else {
            std::memcpy(s, t, 16);
        }
        for (int i = 0; i < 16; i++) s[i] ^= rk[16 * r + i];
    }
    std::memcpy(out, s, 16);
}

static void decrypt(const uint8_t *rk, int nr, const uint8_t in[16], uint8_t out[16]) {
    uint8_t inv_sbox[256];
    for (int x = 0; x < 256; x++) inv_sbox[sbox((uint8_t)x)] = (uint8_t)x;
    uint8_t s[16], t[16];
    for (int i = 0; i < 16; i++) s[i] = in[i] ^ rk[16 * nr + i];
    for (int r = nr - 1; r >= 0; r--) {
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++) t[4 * c + row] = inv_sbox[s[4 * ((c - row) & 3) + row]];
        for (int i = 0; i < 16; i++) t[i] ^= rk[16 * r + i];
        if (r) {
            for (int c = 0; c < 4; c++)
                for (int row = 0; row < 4; row++)
                    s[4 * c + row] = (uint8_t)(mul(t[4 * c + row], 14) ^ mul(t[4 * c + ((row + 1) & 3)], 11) ^
                                               mul(t[4 * c + ((row + 2) & 3)], 13) ^ mul(t[4 * c + ((row + 3) & 3)], 9));
        } else {
            std::memcpy(s, t, 16);
        }
    }
    std::memcpy(out, s, 16);
}

static void word_is(const std::vector<uint8_t> &rk, int i, const char *h) {
    uint8_t w[4];
    hex(h, w, 4);
    CHECK(std::memcmp(&rk[4 * i], w, 4) == 0);
}

int main() {
    static_assert(tae::aes_nk(192) == 6 && tae::aes_nr(192) == 12 && tae::aes_words(192) == 52, "AES-192");
    static_assert(tae::aes_nk(256) == 8 && tae::aes_nr(256) == 14 && tae::aes_words(256) == 60, "AES-256");
    static_assert(tae::aes_words(128) == 44 && !tae::aes_key_bits_ok(160), "AES-128");
    for (int x = 0; x < 256; x++) CHECK(tae::kSbox[x] == sbox((uint8_t)x));

    uint8_t pt[16], want[16], got[16], key[32];
    hex("00112233445566778899aabbccddeeff", pt, 16);
    const char *cts[3] = {"69c4e0d86a7b0430d8cdb78070b4c55a", "dda97ca4864cdfe06eaf70a0ec0d7191",
                          "8ea2b7ca516745bfeafc49904b496089"};  // FIPS-197 C.1, C.2, C.3
    for (int k = 0; k < 3; k++) {
        const int nk = 4 + 2 * k, nr = nk + 6;
        for (int i = 0; i < 4 * nk; i++) key[i] = (uint8_t)i;
        std::vector<uint8_t> rk(16 * (size_t)(nr + 1));  // exactly the bytes the schedule may write
        tae::plain_key_schedule(key, nk, rk.data());
        CHECK(std::memcmp(rk.data(), key, 4 * (size_t)nk) == 0);
        hex(cts[k], want, 16);
        encrypt(rk.data(), nr, pt, got);
        CHECK(std::memcmp(got, want, 16) == 0);
        decrypt(rk.data(), nr, want, got);
        CHECK(std::memcmp(got, pt, 16) == 0);
        if (nk == 4) {
            uint8_t rk128[176];
            tae::plain_key_schedule(key, rk128);  // the 128-bit signature is the same expansion
            CHECK(std::memcmp(rk128, rk.data(), 176) == 0);
        }
    }
    // FIPS-197 appendix A.2 (192 bits) and A.3 (256 bits): w6, w7, w51 and w8, w12, w13, w59
    {
        std::vector<uint8_t> rk(208);
        hex("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b", key, 24);
        tae::plain_key_schedule(key, 6, rk.data());
        word_is(rk, 6, "fe0c91f7");
        word_is(rk, 7, "2402f5a5");
        word_is(rk, 51, "01002202");
    }
    {
        std::vector<uint8_t> rk(240);
        hex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4", key, 32);
        tae::plain_key_schedule(key, 8, rk.data());
        word_is(rk, 8, "9ba35411");
        word_is(rk, 12, "a8b09c1a");
        word_is(rk, 13, "93d194cd");
        word_is(rk, 59, "706c631e");
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
