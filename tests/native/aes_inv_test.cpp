// Host check of the inverse cipher's tables and index helpers (csrc/aes_inv.hpp), following the data flow of
// the device kernels: a muls array [16][4] per round (what the 8 -> 32 circuit bootstrap gives), then the
// combine through inv_mix_src_byte / inv_final_src_byte.  Decrypts the FIPS-197 C.1 vector that way, derives
// the decryption key through the multiples-only table, and checks the three lookup-table functions against
// byte-wise definitions for all 256 inputs.
#include <cstdio>
#include <cstring>

#include "../../tfhe-aes-2_amd/csrc/aes_inv.hpp"

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

// independent definitions: multiplication by repeated xtime (FIPS-197 4.2.1), the S-box from the
// multiplicative inverse and the affine map (5.1.1)
static uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
static uint8_t slow_mul(uint8_t a, uint8_t b) {
    uint8_t r = 0;
    for (int i = 0; i < 8; i++, a = xtime(a))
        if ((b >> i) & 1) r ^= a;
    return r;
}
static uint8_t sbox(uint8_t x) {
    uint8_t inv = 0;
    for (int y = 1; y < 256 && x; y++)
        if (slow_mul(x, (uint8_t)y) == 1) inv = (uint8_t)y;
    uint8_t s = 0x63;
    for (int sh = 0; sh < 5; sh++) s ^= (uint8_t)((inv << sh) | (inv >> (8 - sh)));
    return s;
}

static void key_schedule(const uint8_t key[16], uint8_t rk[176]) {
    static const uint8_t rcon[11] = {0, 1, 2, 4, 8, 16, 32, 64, 128, 0x1b, 0x36};
    std::memcpy(rk, key, 16);
    for (int i = 4; i < 44; i++) {
        uint8_t t[4];
        std::memcpy(t, rk + 4 * (i - 1), 4);
        if (i % 4 == 0) {
            const uint8_t first = t[0];
            t[0] = (uint8_t)(sbox(t[1]) ^ rcon[i / 4]);
            t[1] = sbox(t[2]);
            t[2] = sbox(t[3]);
            t[3] = sbox(first);
        }
        for (int j = 0; j < 4; j++) rk[4 * i + j] = rk[4 * (i - 4) + j] ^ t[j];
    }
}

// multiple m of a 32-bit lookup-table word (MSB first: m = 0 is the top byte)
static uint8_t mul_of(uint32_t word, int m) { return (uint8_t)(word >> (8 * (3 - m))); }

// decryption key through the multiples-only table and the combine without InvShiftRows
static void decrypt_key(const uint8_t rk[176], uint8_t dk[176]) {
    std::memcpy(dk, rk, 176);
    for (int r = 1; r <= 9; r++) {
        uint8_t muls[16][4];
        for (int byte = 0; byte < 16; byte++)
            for (int m = 0; m < 4; m++) muls[byte][m] = mul_of(tae::inv_mul_lut(rk[16 * r + byte]), m);
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++) {
                uint8_t v = 0;
                for (int j = 0; j < 4; j++) v ^= muls[tae::inv_mix_src_byte(row, c, j, false)][j];
                dk[16 * r + tae::inv_byte(row, c)] = v;
            }
    }
}

static void decrypt_block(const uint8_t dk[176], const uint8_t in[16], int rounds, uint8_t out[16]) {
    uint8_t st[16];
    for (int i = 0; i < 16; i++) st[i] = in[i] ^ dk[160 + i];
    for (int r = rounds - 1; r >= 1; r--) {
        uint8_t muls[16][4], next[16];
        for (int byte = 0; byte < 16; byte++)
            for (int m = 0; m < 4; m++) muls[byte][m] = mul_of(tae::inv_sbox_mul_lut(st[byte]), m);
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++) {
                uint8_t v = dk[16 * r + tae::inv_byte(row, c)];
                for (int j = 0; j < 4; j++) v ^= muls[tae::inv_mix_src_byte(row, c, j, true)][j];
                next[tae::inv_byte(row, c)] = v;
            }
        std::memcpy(st, next, 16);
    }
    uint8_t sb[16];
    for (int byte = 0; byte < 16; byte++) sb[byte] = tae::inv_sbox_lut(st[byte]);
    for (int c = 0; c < 4; c++)
        for (int row = 0; row < 4; row++)
            out[tae::inv_byte(row, c)] = sb[tae::inv_final_src_byte(row, c)] ^ dk[tae::inv_byte(row, c)];
}

// the forward cipher with `rounds` rounds (round keys 0, 1..rounds-1, 10), byte-wise
static void encrypt_block(const uint8_t rk[176], const uint8_t in[16], int rounds, uint8_t out[16]) {
    uint8_t st[16];
    for (int i = 0; i < 16; i++) st[i] = in[i] ^ rk[i];
    for (int r = 1; r <= rounds; r++) {
        uint8_t t[16];
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++) t[4 * c + row] = sbox(st[4 * ((c + row) & 3) + row]);
        const bool last = r == rounds;
        for (int c = 0; c < 4; c++)
            for (int row = 0; row < 4; row++) {
                uint8_t v = t[4 * c + row];
                if (!last)
                    v = (uint8_t)(slow_mul(t[4 * c + row], 2) ^ slow_mul(t[4 * c + ((row + 1) & 3)], 3) ^
                                  t[4 * c + ((row + 2) & 3)] ^ t[4 * c + ((row + 3) & 3)]);
                st[4 * c + row] = v ^ rk[(last ? 160 : 16 * r) + 4 * c + row];
            }
    }
    std::memcpy(out, st, 16);
}

int main() {
    // the three lookup-table functions and gf_mul, all 256 inputs
    static const uint8_t coef[4] = {14, 11, 13, 9};
    for (int x = 0; x < 256; x++) {
        CHECK(tae::kInvSbox[sbox((uint8_t)x)] == x);
        CHECK(tae::inv_sbox_lut(sbox((uint8_t)x)) == x);
        for (int m = 0; m < 4; m++) {
            CHECK(tae::kInvMixCoef[m] == coef[m]);
            CHECK(mul_of(tae::inv_mul_lut((uint8_t)x), m) == slow_mul((uint8_t)x, coef[m]));
            CHECK(mul_of(tae::inv_sbox_mul_lut((uint8_t)x), m) == slow_mul(tae::kInvSbox[x], coef[m]));
        }
        for (int y = 0; y < 256; y++) CHECK(tae::gf_mul((uint8_t)x, (uint8_t)y) == slow_mul((uint8_t)x, (uint8_t)y));
    }
    CHECK(tae::gf_mul(0x57, 0x83) == 0xc1);  // FIPS-197 4.2
    // the source-byte helpers are permutations of the 16 bytes per (j) and hit each row once per output
    for (int shift = 0; shift < 2; shift++)
        for (int j = 0; j < 4; j++) {
            int seen = 0;
            for (int c = 0; c < 4; c++)
                for (int row = 0; row < 4; row++) seen |= 1 << tae::inv_mix_src_byte(row, c, j, shift != 0);
            CHECK(seen == 0xffff);
        }
    // FIPS-197 C.1
    uint8_t key[16], pt[16], rk[176], dk[176], out[16];
    static const uint8_t ct[16] = {0x69, 0xc4, 0xe0, 0xd8, 0x6a, 0x7b, 0x04, 0x30,
                                   0xd8, 0xcd, 0xb7, 0x80, 0x70, 0xb4, 0xc5, 0x5a};
    for (int i = 0; i < 16; i++) {
        key[i] = (uint8_t)i;
        pt[i] = (uint8_t)(0x11 * i);
    }
    key_schedule(key, rk);
    encrypt_block(rk, pt, 10, out);
    CHECK(!std::memcmp(out, ct, 16));
    decrypt_key(rk, dk);
    CHECK(!std::memcmp(dk, rk, 16) && !std::memcmp(dk + 160, rk + 160, 16));
    // FIPS-197 C.1 equivalent inverse cipher, round 1's key: dw = 8c56dff0 825dd3f9 805ad3fc 8659d7fd is
    // listed for ik_sch of round 9 = InvMixColumns(rk[1])
    static const uint8_t dw1[16] = {0x8c, 0x56, 0xdf, 0xf0, 0x82, 0x5d, 0xd3, 0xf9,
                                    0x80, 0x5a, 0xd3, 0xfc, 0x86, 0x59, 0xd7, 0xfd};
    CHECK(!std::memcmp(dk + 16, dw1, 16));
    decrypt_block(dk, ct, 10, out);
    CHECK(!std::memcmp(out, pt, 16));
    // every round count inverts the forward cipher of that count
    for (int rounds = 1; rounds <= 10; rounds++) {
        uint8_t e[16];
        encrypt_block(rk, pt, rounds, e);
        decrypt_block(dk, e, rounds, out);
        CHECK(!std::memcmp(out, pt, 16));
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
