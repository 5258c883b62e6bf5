// AES-128 constants and byte-level helpers used by the FHE round driver.
// Reference: src/aes_128.rs (SBOX :18-35, RC :37-39, ROUNDS :16, gf_256_mul :42-56),
// src/aes_128/plain.rs:106-132 (key schedule, for host-side checks).
#pragma once
#include <cstdint>

namespace tae {

extern const uint8_t kSbox[256];
extern const uint8_t kRcon[11];
constexpr int kAesRounds = 10;  // AES-128, the default everywhere

// FIPS-197 figure 4 for key_bits = 128 / 192 / 256: Nk key words, Nr = Nk + 6 rounds, 4 (Nr + 1) expanded words
// (44 / 52 / 60).  kRcon's 11 entries cover every size (the last index used is 10, 8 and 7).
constexpr bool aes_key_bits_ok(int key_bits) { return key_bits == 128 || key_bits == 192 || key_bits == 256; }
constexpr int aes_nk(int key_bits) { return key_bits / 32; }
constexpr int aes_nr(int key_bits) { return key_bits / 32 + 6; }
constexpr int aes_words(int key_bits) { return 4 * (aes_nr(key_bits) + 1); }

// gf_256_mul exactly as the reference writes it, including its reduction quirk (it XORs 0x1b
// when the high bit is CLEAR, aes_128.rs:50).  The x2/x3 LUT outputs inherit the quirk; the two
// 0x1b terms cancel inside every MixColumns output, so full AES stays correct.
uint8_t gf_256_mul(uint8_t a, uint8_t b);

// fhe_sbox_pbs::gf_256_mul (fhe_sbox_pbs.rs:33-53) on bits: the byte is shifted and XORed bit by
// bit (MSB-first, reduce by x^8 = x^4 + x^3 + x + 1).  terms[o][i] = how often input bit i is added
// into output bit o (LWE additions: nothing cancels).  mix_column_terms: MixColumns (:56-73) as
// a 32 x 32 map on one column, out byte r = 2 s_r + s_{r+3} + s_{r+2} + 3 s_{r+1}.
void gf_256_mul_bit_terms(uint8_t b, int terms[8][8]);
void mix_column_terms(int terms[32][32]);

// plain key expansion into 176 bytes (word-major), plain.rs:106-132
void plain_key_schedule(const uint8_t key[16], uint8_t rk[176]);
// FIPS-197 5.2 for nk = 4 / 6 / 8 key words: key [4 nk] -> rk [16 (nk + 7)] bytes
void plain_key_schedule(const uint8_t *key, int nk, uint8_t *rk);

}  // namespace tae
