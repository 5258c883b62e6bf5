/*
 * tfhe_aes_gpu.h -- C-ABI of the MI355X-native FHE AES-128 evaluator (drop-in boundary).
 *
 * Plain C types only (opaque handles, pointers, sizes, int status codes); no torch/HIP types.
 * Every entry point names the reference interface it replaces (allanbrondum/tfhe-aes-2 @
 * 2025-03-07, paths relative to the reference root).  The reference is in-process Rust; these
 * are the symbols a Rust `extern "C"` shim implementing its traits would bind.
 *
 * Conventions
 *   - LWE ciphertexts are u64 arrays in the tfhe layout [a_0 .. a_{K-1}, b] (K = k*N, big key);
 *     a byte is 8 ciphertexts MSB-first (src/util.rs:33-42); a block is 16 bytes in block order;
 *     an expanded key is 44 words x 4 bytes (fhe.rs:16-38, [Word; 44]).
 *   - Errors are status codes instead of the reference's panics; tae_last_error() gives the
 *     message of the calling thread's last failure.
 *   - A context is bound to one GPU and internally serialised: safe to share across host
 *     threads (the reference's FheContext is Send + Sync).
 *   - There is no CPU fallback: without a usable GPU, context creation fails with TAE_E_NODEV.
 */
#ifndef TFHE_AES_GPU_H
#define TFHE_AES_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (the reference panics: "NoiseTooBig", "noise components not independent") */
#define TAE_OK 0
#define TAE_E_NOISE 1     /* MaxNoiseLevel::validate -> NoiseTooBig (shortint_woppbs_1bit.rs:74-76) */
#define TAE_E_INDEP 2     /* "noise components not independent" (shortint_woppbs_1bit.rs:64-70) */
#define TAE_E_PARAM 3     /* invalid parameter / unsupported shape */
#define TAE_E_HIP 4       /* HIP runtime failure */
#define TAE_E_ARG 5       /* invalid argument (null pointer, size mismatch) */
#define TAE_E_NODEV 6     /* no GPU available: the product path has no CPU fallback */

/* parameter sets: src/tfhe/shortint_woppbs_1bit/parameters.rs */
#define TAE_PARAMS_SQRD_LVL_1 0   /* :29-61  */
#define TAE_PARAMS_SQRD_LVL_4 1   /* :77-109 */
#define TAE_PARAMS_SQRD_LVL_64 2  /* :125-157, default (bin/main.rs:82-83) */
#define TAE_PARAMS_SQRD_LVL_256 3 /* :173-205 */
/* the 8-bit model's set: src/tfhe/shortint_woppbs_8bit.rs:39-86 (ShortintWoppbs8BitSboxPbsAesEncrypt,
 * fhe_impls/shortint_woppbs_8bit.rs:44-64).  Bits are LWEs under the SMALL key ([n+1] u64); a byte
 * is bootstrapped through one 8-bit integer ciphertext (big key, [K+1], plaintext m * 2^56). */
#define TAE_PARAMS_WOPPBS_8BIT 4
/* the shortint_1bit model's set: src/tfhe/shortint_1bit.rs:62-83 (ClassicPBSParameters, message modulus 2,
 * carry 1, EncryptionKeyChoice::Small; Shortint1BitSboxPbsAesEncrypt, fhe_impls/shortint_1bit.rs:52-72).
 * Bits are shortint ciphertexts under the SMALL key ([n+1] u64, plaintext m * 2^62); the third server key
 * array ("pfpksk") holds the packing keyswitch key [n][ks_l][(k+1)N] (shortint_1bit.rs:176-186). */
#define TAE_PARAMS_SHORTINT_1BIT 5

/* memory kinds for the raw-array entry points.  TAE_MEM_DEVICE: pointers into the context's device
 * memory.  By default the library orders itself after all work already queued on that device (it
 * synchronizes the device before its first read of caller buffers, e.g. after an RCCL broadcast or torch
 * copies on other streams); after tae_set_caller_stream it waits only for the work queued on that one
 * stream (an event, no host sync).  Device outputs are complete when the call returns. */
#define TAE_MEM_HOST 0
#define TAE_MEM_DEVICE 1

typedef struct tae_client_key tae_client_key; /* shortint_woppbs_1bit::ClientKey (:189-195) */
typedef struct tae_context tae_context;       /* shortint_woppbs_1bit::FheContext (:165-172) */
typedef struct tae_bit tae_bit;               /* shortint_woppbs_1bit::BitCt (:26-32) */
typedef struct tae_lut tae_lut;               /* tfhe::shortint::wopbs::WopbsLUTBase */

typedef struct {
    int n, k, N, pbs_l, pbs_b, ks_l, ks_b, cbs_l, cbs_b, pfks_l, pfks_b;
    double lwe_std, glwe_std, pfks_std;
    uint64_t max_noise_sq; /* 1-bit model: max noise^2; 8-bit model: shortint MaxNoiseLevel (11) */
    int model;             /* 1 = shortint_woppbs_1bit, 8 = shortint_woppbs_8bit */
} tae_params;

const char *tae_last_error(void);
const char *tae_version(void);
int tae_device_count(int *count);
int tae_get_params(int param_set, tae_params *out); /* parameters::params_sqrd_lvl_* */
/* u64 length of one bit ciphertext: K+1 (1-bit model, big key) or n+1 (8-bit model, small key) */
int tae_bit_len(int param_set, size_t *len);

/* ---- keys (FheContext::generate_keys_with_params, shortint_woppbs_1bit.rs:245-268) ----------
 * Client key generation on the host from a 32-byte seed (ChaCha20 streams, DESIGN.md keygen
 * spec), server keys uploaded to `device` and the bootstrapping key converted to the Fourier
 * domain there.  generate_keys_sqrd_lvl_* (:229-243) = this with the matching param_set. */
int tae_generate_keys(int param_set, const uint8_t seed[32], int device, int threads,
                      tae_client_key **client_key, tae_context **context);
/* Client key only + standard-domain server keys exported to caller buffers (sizes from
 * tae_server_key_sizes) -- used to broadcast keys across ranks before tae_context_create_raw. */
int tae_server_key_sizes(int param_set, size_t *ksk_len, size_t *bsk_len, size_t *pfpksk_len);
int tae_generate_keys_raw(int param_set, const uint8_t seed[32], int threads,
                          tae_client_key **client_key, uint64_t *ksk, uint64_t *bsk,
                          uint64_t *pfpksk);
/* Client key only (secret keys from the seed's LWE_SK / GLWE_SK streams; no server keys) -- every rank
 * of a multi-GPU run derives the same client key this way while server keys are broadcast. */
int tae_client_key_from_seed(int param_set, const uint8_t seed[32], tae_client_key **client_key);
/* Server context from raw keys: mem = TAE_MEM_HOST (copied to the device) or TAE_MEM_DEVICE
 * (device pointers on `device`, e.g. after an RCCL broadcast; they must outlive the context). */
int tae_context_create_raw(int param_set, int device, const uint64_t *ksk, const uint64_t *bsk,
                           const uint64_t *pfpksk, int mem, tae_context **context);
void tae_context_free(tae_context *ctx);

/* ---- On-disk keys (no reference counterpart: the reference keeps keys in memory) --
 * One little-endian file "TAEKEY02" holding a client key (its 32-byte seed + encryption counter)
 * and/or the standard-domain server keys (ksk, bsk, pfpksk as sized by tae_server_key_sizes), with
 * a trailing checksum (format: tfhe-aes-2_amd/csrc/keyio.cpp).  Rejected files -> TAE_E_ARG. */
#define TAE_KEYS_CLIENT 1
#define TAE_KEYS_SERVER 2
/* client_key may be NULL; ksk/bsk/pfpksk all NULL (client only) or all set */
int tae_keys_save(const char *path, int param_set, const tae_client_key *client_key, const uint64_t *ksk,
                  const uint64_t *bsk, const uint64_t *pfpksk);
/* parameter set and TAE_KEYS_* flags from the header (payload not verified) */
int tae_keys_file_info(const char *path, int *param_set, int *flags);
/* client_key (NULL: not wanted) and/or the three server arrays (all NULL: not wanted); the checksum
 * is verified before anything is returned (server arrays are filled in place: discard them on error) */
int tae_keys_load(const char *path, tae_client_key **client_key, uint64_t *ksk, uint64_t *bsk, uint64_t *pfpksk);
void tae_client_key_free(tae_client_key *ck);
int tae_client_key_secrets(const tae_client_key *ck, uint64_t *lwe_sk /*[n]*/,
                           uint64_t *glwe_sk /*[k*N]*/);
int tae_context_params(const tae_context *ctx, tae_params *out);

/* ---- ClientKeyT / ContextT (src/tfhe.rs:11-24) -------------------------------------------- */
int tae_encrypt(const tae_client_key *ck, uint64_t bit, tae_bit **out);       /* ClientKey::encrypt */
int tae_decrypt(const tae_client_key *ck, const tae_bit *bit, uint64_t *out); /* ClientKey::decrypt */
int tae_trivial(const tae_context *ctx, uint64_t bit, tae_bit **out);         /* ContextT::trivial */
/* raw: encrypt `count` bits ([count][K+1]) with encryption indices start..start+count-1.  Each index
 * selects the ciphertext's mask and noise streams (DESIGN.md keygen spec), so an index must never be
 * reused for a different plaintext under one key: explicit ranges must lie below 2^63 (TAE_E_ARG
 * otherwise); start_index = TAE_INDEX_AUTO reserves `count` fresh indices from the key's counter,
 * the region tae_encrypt draws from (disjoint from every explicit range). */
#define TAE_INDEX_AUTO UINT64_MAX
int tae_encrypt_bits_raw(const tae_client_key *ck, const uint8_t *bits, size_t count,
                         uint64_t start_index, uint64_t *out);
int tae_decrypt_bits_raw(const tae_client_key *ck, const uint64_t *cts, size_t count, uint8_t *bits);
/* 8-bit model integers (FullWidthCiphertext, shortint_woppbs_8bit.rs:167-178): shortint
 * encrypt_without_padding / decrypt_without_padding, message modulus 256 ([count][K+1]) */
int tae_encrypt_ints_raw(const tae_client_key *ck, const uint8_t *values, size_t count, uint64_t start_index,
                         uint64_t *out);
int tae_decrypt_ints_raw(const tae_client_key *ck, const uint64_t *cts, size_t count, uint8_t *values);

/* ---- BitCt (shortint_woppbs_1bit.rs:26-151) ----------------------------------------------- */
int tae_bit_clone(const tae_bit *bit, tae_bit **out);
void tae_bit_free(tae_bit *bit);
int tae_bit_xor_assign(tae_bit *lhs, const tae_bit *rhs); /* BitXorAssign (:134-142) */
int tae_bit_noise_level(const tae_bit *bit, uint64_t *noise_level_squared);
int tae_bit_data(const tae_bit *bit, uint64_t *out, size_t len); /* LWE coefficients [K+1] */
int tae_bit_from_data(const tae_context *ctx, const uint64_t *data, size_t len,
                      uint64_t noise_level_squared, tae_bit **out); /* BitCt::with_noise_level */
/* BitXorAssign over whole arrays of bits (xor_state, src/aes_128/fhe/data_model.rs:270-274):
 * lhs[i] += rhs[i] (wrapping u64 LWE addition = XOR of the encoded bits) for `count` bit ciphertexts
 * of tae_bit_len words each, on the context's GPU.  With both noise arrays (squared noise levels per
 * bit) the reference's NoiseTooBig rule is enforced before anything is written and out_noise_sq
 * (may be NULL) receives the sums; the component-independence check needs BitCt handles
 * (tae_bit_xor_assign) and is the caller's duty here.  The three noise arrays are always HOST
 * pointers, whatever `mem` says (mem applies to lhs / rhs only). */
int tae_xor_batch(const tae_context *ctx, uint64_t *lhs, const uint64_t *rhs, size_t count,
                  const uint64_t *lhs_noise_sq, const uint64_t *rhs_noise_sq, uint64_t *out_noise_sq, int mem);

/* ---- LUT + circuit bootstrap (shortint_woppbs_1bit.rs:274-336) ----------------------------- */
/* generate_lookup_table: f_values[1 << input_bits] */
int tae_generate_lookup_table(const tae_context *ctx, int input_bits, int output_bits,
                              const uint64_t *f_values, tae_lut **out);
void tae_lut_free(tae_lut *lut);
/* generate_multivariate_luts (shortint_woppbs_1bit.rs:366-403) without a context, for any power-of-two
 * polynomial size: out [output_bits][poly_size << max(0, input_bits - log2 poly_size)], small LUT j
 * holding encode_bit(bit output_bits-1-j of f(v)) at coefficient v (the layout pinned by the
 * reference's tests :665-697); out_len must equal that size.  input_bits is 1..16 as in the reference
 * (its assert 0 < input_bits <= 16 and u16 argument of f, :372); anything else is TAE_E_ARG. */
int tae_generate_multivariate_luts(int poly_size, int input_bits, int output_bits, const uint64_t *f_values,
                                   uint64_t *out, size_t out_len);
int tae_lut_data(const tae_lut *lut, uint64_t *out, size_t len, size_t *needed);
/* FheContext::circuit_bootstrap(&[&BitCt], &WopbsLUTBase) -> Vec<BitCt> */
int tae_circuit_bootstrap(const tae_context *ctx, const tae_bit *const *bits, size_t n_bits,
                          const tae_lut *lut, tae_bit **out /*[output_bits]*/);
/* batched: groups x n_in bits [groups][n_in][K+1] -> [groups][n_out][K+1] */
int tae_circuit_bootstrap_raw(const tae_context *ctx, const uint64_t *bits, size_t groups,
                              int n_in, const tae_lut *lut, uint64_t *out, int mem);

/* ---- 8-bit model FheContext (shortint_woppbs_8bit.rs:262-336) ------------------------------
 * generate_lookup_table: tae_generate_lookup_table(ctx, 8, 8, f[256]) (without-padding LUT);
 * tae_circuit_bootstrap[_raw] with n_in = 8 runs Byte::bootstrap_with_lut (8 bits -> 8 bits).
 * bootstrap_from_bits: bits [groups][8][n+1] -> ints [groups][K+1] */
int tae_bootstrap_from_bits_raw(const tae_context *ctx, const uint64_t *bits, size_t groups, const tae_lut *lut,
                                uint64_t *out, int mem);
/* extract_bits_from_ciphertext: ints [groups][K+1] -> bits [groups][8][n+1], MSB first */
int tae_extract_bits_raw(const tae_context *ctx, const uint64_t *ints, size_t groups, uint64_t *out, int mem);

/* ---- shortint_1bit model (context of TAE_PARAMS_SHORTINT_1BIT; src/tfhe/shortint_1bit.rs) -------------- */
/* Test vectors are GLWE ciphertexts [(k+1)N] u64 and always host arrays; bits are [n+1] (mem applies). */
/* FheContext::test_vector_from_cleartext_fn (:208-223, :365-390) for f(0) = f0, f(1) = f1 */
int tae_s1_test_vector_from_fn(int param_set, uint64_t f0, uint64_t f1, uint64_t *tv);
/* FheContext::bootstrap (:257-294, :296-350) over count bits: bit b is bootstrapped with tvs[b % n_tv] */
int tae_s1_bootstrap(const tae_context *ctx, const uint64_t *in, size_t count, const uint64_t *tvs, size_t n_tv,
                     uint64_t *out, int mem);
/* FheContext::packing_keyswitch (:240-255, :494-518): count (1..N) bits -> one GLWE, bit j at coefficient j */
int tae_s1_packing_keyswitch(const tae_context *ctx, const uint64_t *cts, size_t count, uint64_t *glwe, int mem);
/* FheContext::test_vector_from_ciphertexts (:225-238, :392-492) for count pairs: tvs [count][(k+1)N] (mem) */
int tae_s1_test_vectors_from_ciphertexts(const tae_context *ctx, const uint64_t *ct0, const uint64_t *ct1, size_t count,
                                         uint64_t *tvs, int mem);
/* calculate_multivariate_function (:539-583) with generate_multivariate_test_vector (:520-537) for n_fn
 * functions f_tables [n_fn][2^nbits] (host, 0/1, index = bits MSB first) of each of `groups` groups of
 * nbits (1..8) bits [groups][nbits][n+1] -> out [groups][n_fn][n+1] (ByteT::sbox_substitute is 8
 * functions of a byte, fhe_impls/shortint_1bit.rs:32-50) */
int tae_s1_multivariate(const tae_context *ctx, const uint64_t *bits, size_t groups, int nbits,
                        const uint64_t *f_tables, int n_fn, uint64_t *out, int mem);

/* ---- Aes128Encrypt for ShortintWoppbs1BitSboxGalMulPbsAesEncrypt -------------------------
 *      (src/aes_128/fhe.rs:16-38, fhe_impls/shortint_woppbs_1bit.rs:131-151,
 *       fhe_sbox_gal_mul_pbs.rs:84-191) */
/* encrypt_block_for_rounds: expanded_key[44*32] bits, block[128] bits, out[128] */
int tae_aes_encrypt_block_for_rounds(const tae_context *ctx, const tae_bit *const *expanded_key,
                                     const tae_bit *const *block, int rounds, tae_bit **out);
/* batched extension of encrypt_block (main.rs:141-159 runs blocks in parallel) */
int tae_aes_encrypt_blocks(const tae_context *ctx, const tae_bit *const *expanded_key,
                           const tae_bit *const *blocks, size_t n_blocks, int rounds, tae_bit **out);
/* key_schedule (fhe_sbox_gal_mul_pbs.rs:134-164): key[128] bits -> expanded[44*32] bits */
int tae_aes_key_schedule(const tae_context *ctx, const tae_bit *const *key, tae_bit **expanded);
/* raw arrays: rk [44*32][L], blocks [n][128][L], out [n][128][L] with L = tae_bit_len (K+1, or
 * n+1 for the 8-bit model's ShortintWoppbs8BitSboxPbsAesEncrypt / fhe_sbox_pbs.rs:75-121); inputs
 * fresh (noise level 1) -- the noise schedule of the round function is validated statically. */
int tae_aes_encrypt_blocks_raw(const tae_context *ctx, const uint64_t *rk, const uint64_t *blocks,
                               size_t n_blocks, int rounds, uint64_t *out, int mem);
/* key_schedule on raw fresh key bits [128][L] -> [44*32][L] (either model) */
int tae_aes_key_schedule_raw(const tae_context *ctx, const uint64_t *key, uint64_t *expanded, int mem);

/* ---- AES-128-CTR with public counters: transciphering (src/bin/main.rs:108-128) -------------------
 * Counter block i is iv[8] || be64(first_counter + i) (main.rs:108-115 counts from 1); a range that wraps
 * past 2^64 - 1 is TAE_E_ARG.  The iv and the counters are public, so the server needs no counter
 * ciphertexts: round 0 is built from rk0 and the public bytes, and round 1 is bootstrapped once per
 * distinct (byte position, byte value) pair and shared between the blocks, giving the words
 * tae_aes_encrypt_blocks_raw gives on trivial encryptions of the counter blocks.  Parameter sets:
 * TAE_PARAMS_SQRD_LVL_* (gal-mul driver) and TAE_PARAMS_WOPPBS_8BIT; TAE_PARAMS_SHORTINT_1BIT is
 * TAE_E_PARAM.  The noise schedule is validated statically, before any device work. */
/* number of round-1 SBOX groups of the range (host only, no context): 8 for the iv + the distinct values
 * of each counter byte; 0 for n_blocks == 0 */
int tae_aes_ctr_plan(const uint8_t iv[8], uint64_t first_counter, size_t n_blocks, size_t *round1_groups);
/* keystream blocks: out [n_blocks][128][L]; rk [44*32][L]; rk/out follow `mem`, iv is a host pointer.
 * n_blocks == 0 is TAE_OK and writes nothing.  Calls above TAE_CTR_CHUNK_BLOCKS (default 1024, read at
 * context creation) blocks run in consecutive chunks; the result does not depend on the chunk size. */
int tae_aes_ctr_keystream_raw(const tae_context *ctx, const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter,
                              size_t n_blocks, int rounds, uint64_t *out, int mem);
/* data: AES-128-CTR ciphertext bytes (host); out [len][8][L] = FHE encryptions of the plaintext bits, 10 rounds
 * (keystream bit + data bit << 63 on the body; main.rs:117-128 XORs the decrypted keystream instead).
 * len need not be a multiple of 16; len == 0 is TAE_OK and writes nothing. */
int tae_aes_ctr_transcipher_raw(const tae_context *ctx, const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter,
                                const uint8_t *data, size_t len, uint64_t *out, int mem);
/* the same on handles: out[len*8] new bits carrying the round function's noise bookkeeping */
int tae_aes_ctr_transcipher(const tae_context *ctx, const tae_bit *const *expanded_key, const uint8_t iv[8],
                            uint64_t first_counter, const uint8_t *data, size_t len, tae_bit **out /*[len*8]*/);

/* ---- AES-128 inverse cipher and CBC transciphering (FIPS-197 section 5.3) ---------------------------
 * The reference has no decryption and no counterpart of these functions; they are FIPS-197 5.3 (in the
 * order of 5.3.5) in this library's conventions.  InvSubBytes and InvMixColumns' Galois multiples
 * {14, 11, 13, 9} (true products modulo 0x11b) come from one 8 -> 32 circuit bootstrap per byte and middle
 * round, the last round from one 8 -> 8: `rounds` bootstraps per block, as encryption.
 * tae_aes_decrypt_blocks(rounds) inverts tae_aes_encrypt_blocks(rounds) (round keys 10, rounds-1 .. 1, 0).
 * Parameter sets: TAE_PARAMS_SQRD_LVL_* (gal-mul driver) only; TAE_PARAMS_WOPPBS_8BIT and
 * TAE_PARAMS_SHORTINT_1BIT are TAE_E_PARAM.  Raw entry points validate the noise schedule statically,
 * before any device work; handle entry points propagate it per bit. */
/* FIPS-197 5.3.5 decryption key (no reference counterpart): dk [44*32] laid out like the expanded key; words
 * 0..3 and 40..43 are copies, words 4r..4r+3 (r = 1..9) = InvMixColumns(rk[r]), derived on the device by one
 * 8 -> 32 bootstrap of the 144 bytes, the 4-term sums and one identity bootstrap of the 1152 bits
 * (noise^2 = 1, new ids). */
int tae_aes_decrypt_key(const tae_context *ctx, const tae_bit *const *expanded_key, tae_bit **dk /*[44*32]*/);
/* FIPS-197 5.3.5 decryption key on raw arrays (no reference counterpart): rk, dk [44*32][L] follow `mem`;
 * with TAE_MEM_DEVICE dk must not be rk */
int tae_aes_decrypt_key_raw(const tae_context *ctx, const uint64_t *rk, uint64_t *dk, int mem);
/* FIPS-197 5.3 inverse cipher on handles (no reference counterpart): blocks, out [n_blocks*128]; feeding
 * tae_aes_encrypt_blocks' output back with a key derived from the same expanded key is TAE_E_INDEP (the
 * output carries round key 10's ids) */
int tae_aes_decrypt_blocks(const tae_context *ctx, const tae_bit *const *dk, const tae_bit *const *blocks,
                           size_t n_blocks, int rounds, tae_bit **out);
/* FIPS-197 5.3 inverse cipher on raw arrays (no reference counterpart): dk [44*32][L], blocks / out
 * [n_blocks][128][L], all following `mem` */
int tae_aes_decrypt_blocks_raw(const tae_context *ctx, const uint64_t *dk, const uint64_t *blocks, size_t n_blocks,
                               int rounds, uint64_t *out, int mem);
/* CBC decryption of a public ciphertext, FIPS-197 5.3 per block (no reference counterpart): out[len*8] =
 * encryptions of P_i = Dec(C_i) ^ C_{i-1}, C_{-1} = iv, 10 rounds.  len % 16 != 0 is TAE_E_ARG, len == 0 is
 * TAE_OK and writes nothing; padding is the client's business.  No input ciphertexts are made: round 0 is
 * dk[40..43] + the public bits, and the last step adds the public bits of C_{i-1} (no noise). */
int tae_aes_cbc_transcipher(const tae_context *ctx, const tae_bit *const *dk, const uint8_t iv[16], const uint8_t *data,
                            size_t len, tae_bit **out /*[len*8]*/);
/* the same on raw arrays (FIPS-197 5.3, no reference counterpart): dk / out [len][8][L] follow `mem`; iv and
 * data are host pointers */
int tae_aes_cbc_transcipher_raw(const tae_context *ctx, const uint64_t *dk, const uint8_t iv[16], const uint8_t *data,
                                size_t len, uint64_t *out, int mem);
/* noise bookkeeping of the FIPS-197 5.3 inverse cipher for fresh inputs (no reference counterpart; no GPU):
 * the decryption-key derivation, then `rounds` rounds with the derived key.  TAE_OK, TAE_E_NOISE or
 * TAE_E_INDEP; parameter sets other than TAE_PARAMS_SQRD_LVL_* and rounds outside 1..=10 are TAE_E_PARAM */
int tae_aes_decrypt_noise_schedule_check(int param_set, int rounds);

/* ---- AES-128 / 192 / 256 by key size (FIPS-197 section 5.2 and figure 11) ---------------------------
 * The reference is AES-128 only and has no counterpart of these functions; they are the tae_aes_* entry
 * points above with `key_bits` after the context.  key_bits = 128 / 192 / 256 (anything else is TAE_E_PARAM)
 * gives Nk = key_bits / 32 key words, Nr = Nk + 6 = 10 / 12 / 14 rounds and W = 4 (Nr + 1) = 44 / 52 / 60
 * expanded words; every expanded or decryption key below is [W*32] bits in the layout of tae_aes_*, a handle
 * array of another length is TAE_E_ARG, and `rounds` outside 1..=Nr is TAE_E_PARAM.  A run of `rounds` rounds
 * uses round keys 0, 1..rounds-1 and Nr; the inverse uses Nr, rounds-1..1, 0.  The modes take `rounds` where
 * their tae_aes_* namesakes fix 10.  Parameter sets: TAE_PARAMS_SQRD_LVL_* (gal-mul driver); 192 and 256 on
 * TAE_PARAMS_WOPPBS_8BIT and TAE_PARAMS_SHORTINT_1BIT are TAE_E_PARAM.  With key_bits = 128 the cipher and
 * the modes are the tae_aes_* paths themselves. */
/* FIPS-197 figure 4 (no reference counterpart; no GPU): the number of expanded words W of a key size */
int tae_aesx_expanded_words(int key_bits, size_t *words);
/* FIPS-197 5.2 key expansion on handles (no reference counterpart): key[key_bits] bits -> expanded[W*32]; runs
 * on the device, words from Nk on come out of an identity bootstrap (noise^2 = 1, new ids) */
int tae_aesx_key_schedule(const tae_context *ctx, int key_bits, const tae_bit *const *key, tae_bit **expanded);
/* FIPS-197 5.2 key expansion on raw fresh key bits [key_bits][L] -> [W*32][L] (no reference counterpart); with
 * TAE_MEM_DEVICE no ciphertext leaves the device; at 128 bits the words equal tae_aes_key_schedule_raw's */
int tae_aesx_key_schedule_raw(const tae_context *ctx, int key_bits, const uint64_t *key, uint64_t *expanded, int mem);
/* FIPS-197 5.1 cipher on handles, figure 11 key sizes (no reference counterpart): blocks, out [n_blocks*128] */
int tae_aesx_encrypt_blocks(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                            const tae_bit *const *blocks, size_t n_blocks, int rounds, tae_bit **out);
/* FIPS-197 5.1 cipher on raw arrays (no reference counterpart): rk [W*32][L], blocks / out [n_blocks][128][L] */
int tae_aesx_encrypt_blocks_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint64_t *blocks,
                                size_t n_blocks, int rounds, uint64_t *out, int mem);
/* tae_aes_ctr_keystream_raw with a FIPS-197 figure 11 key size (no reference counterpart): rk [W*32][L] */
int tae_aesx_ctr_keystream_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint8_t iv[8],
                               uint64_t first_counter, size_t n_blocks, int rounds, uint64_t *out, int mem);
/* tae_aes_ctr_transcipher_raw with a FIPS-197 figure 11 key size and `rounds` (no reference counterpart) */
int tae_aesx_ctr_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint8_t iv[8],
                                 uint64_t first_counter, const uint8_t *data, size_t len, int rounds, uint64_t *out,
                                 int mem);
/* tae_aes_ctr_transcipher with a FIPS-197 figure 11 key size and `rounds` (no reference counterpart) */
int tae_aesx_ctr_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                             const uint8_t iv[8], uint64_t first_counter, const uint8_t *data, size_t len, int rounds,
                             tae_bit **out /*[len*8]*/);
/* FIPS-197 5.3.5 decryption key on handles (no reference counterpart): words 0..3 and 4Nr..4Nr+3 are copies,
 * words 4r..4r+3 (r = 1..Nr-1) = InvMixColumns(rk[r]) with noise^2 = 1 and new ids */
int tae_aesx_decrypt_key(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key, tae_bit **dk);
/* FIPS-197 5.3.5 decryption key on raw arrays (no reference counterpart): rk, dk [W*32][L]; dk must not be rk */
int tae_aesx_decrypt_key_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, uint64_t *dk, int mem);
/* FIPS-197 5.3 inverse cipher on handles (no reference counterpart); TAE_E_INDEP as tae_aes_decrypt_blocks */
int tae_aesx_decrypt_blocks(const tae_context *ctx, int key_bits, const tae_bit *const *dk, const tae_bit *const *blocks,
                            size_t n_blocks, int rounds, tae_bit **out);
/* FIPS-197 5.3 inverse cipher on raw arrays (no reference counterpart): dk [W*32][L] */
int tae_aesx_decrypt_blocks_raw(const tae_context *ctx, int key_bits, const uint64_t *dk, const uint64_t *blocks,
                                size_t n_blocks, int rounds, uint64_t *out, int mem);
/* tae_aes_cbc_transcipher with a FIPS-197 figure 11 key size and `rounds` (no reference counterpart) */
int tae_aesx_cbc_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *dk, const uint8_t iv[16],
                             const uint8_t *data, size_t len, int rounds, tae_bit **out /*[len*8]*/);
/* tae_aes_cbc_transcipher_raw with a FIPS-197 figure 11 key size and `rounds` (no reference counterpart) */
int tae_aesx_cbc_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *dk, const uint8_t iv[16],
                                 const uint8_t *data, size_t len, int rounds, uint64_t *out, int mem);
/* noise bookkeeping for a fresh key and block (FIPS-197 5.2, then 5.1 or 5.3; no reference counterpart; no GPU):
 * the key expansion, then `rounds` cipher rounds, or with inverse != 0 the decryption-key derivation and `rounds`
 * inverse rounds.  TAE_OK, TAE_E_NOISE or TAE_E_INDEP; other models than the 1-bit one are TAE_E_PARAM */
int tae_aesx_noise_schedule_check(int param_set, int key_bits, int rounds, int inverse);

/* ---- XTS-AES decryption of a public ciphertext (IEEE 1619 / NIST SP 800-38E) ---------
 * The reference has no XTS and no counterpart of these functions.  Data at rest: the server holds the
 * decryption key of K1 (tae_aesx_decrypt_key) and the expanded key of K2 under FHE, one key_bits for both
 * (XTS-AES-128 is two 16-byte keys, XTS-AES-256 two 32-byte keys), and the ciphertext in the clear.  For a data
 * unit the tweak is 16 public bytes (the unit number, little-endian, in IEEE 1619); block j of the unit is
 *     P_j = Dec_K1(C_j ^ M_j) ^ M_j,   M_j = alpha^j T,   T = Enc_K2(tweak),
 * alpha^j being the multiplication by x^j in GF(2^128) modulo x^128 + x^7 + x^2 + x + 1 with coefficient k at
 * bit k & 7 (from the LSB) of byte k >> 3.  T is refreshed by one identity bootstrap (noise^2 = 1, new ids), a
 * mask bit is the LWE sum of the tweak bits in its row of the GF(2) matrix of alpha^j and has noise^2 = its row
 * weight <= w(j), and an output bit has 8 + 1 + its row weight: a call with a block index whose 9 + w(j) is above
 * the parameter set's cap (w(j) > 55 at TAE_PARAMS_SQRD_LVL_64) is TAE_E_NOISE before any device work.  w(j) is
 * not monotonic: it is at most 9 below block 256 (4 KiB units) and first exceeds 55 at block 1721.  `rounds` (1..=Nr) applies to both ciphers.  Scope of tae_aesx_* decryption: TAE_PARAMS_SQRD_LVL_*,
 * gal-mul driver; the other models are TAE_E_PARAM.  Ciphertext stealing is not supported: a unit's len must be a
 * positive multiple of 16, else TAE_E_PARAM.  Arguments are checked first; then a machine without a GPU answers
 * TAE_E_NODEV. */
/* one data unit, or a range of its blocks (no reference counterpart): `data` is the ciphertext from block
 * first_block of the unit on, len bytes */
typedef struct {
    uint8_t tweak[16];
    uint64_t first_block;
    const uint8_t *data;
    size_t len;
} tae_xts_unit;
/* w(j), the largest row weight of the GF(2) matrix of alpha^j (no reference counterpart; no GPU) */
int tae_aesx_xts_row_weight(uint64_t block_index, int *weight);
/* noise bookkeeping of XTS decryption for fresh keys (no reference counterpart; no GPU): both key expansions, the
 * decryption key of K1, the tweak cipher with its refresh, and block max_block_index of a unit, that block alone
 * (w(j) is not monotonic; the compute calls check every block index they are given).  TAE_OK or TAE_E_NOISE;
 * other models than the 1-bit one are TAE_E_PARAM */
int tae_aesx_xts_noise_schedule_check(int param_set, int key_bits, int rounds, uint64_t max_block_index);
/* T = Enc_K2(tweak) for n tweaks, each refreshed by the identity bootstrap (no reference counterpart): rk2
 * [W*32][L] and out [n][128][L] follow `mem`, tweaks [n][16] is a host pointer.  Equal tweaks are computed once and
 * come out as identical words */
int tae_aesx_xts_tweaks_raw(const tae_context *ctx, int key_bits, const uint64_t *rk2, const uint8_t *tweaks /*[n][16]*/,
                            size_t n, int rounds, uint64_t *out /*[n][128][L]*/, int mem);
/* the mask stage alone (no reference counterpart): masks [nb][128][L], block b = alpha^block_index[b] applied to
 * the tweak ciphertexts of unit unit_of_block[b] of tweaks_ct [n_units][128][L]; the two index arrays are host
 * pointers, a unit outside 0..n_units-1 is TAE_E_ARG.  A stage call: no noise rule is applied */
int tae_stage_xts_masks(const tae_context *ctx, const uint64_t *tweaks_ct, size_t n_units, const int32_t *unit_of_block,
                        const uint64_t *block_index, size_t nb, uint64_t *masks, int mem);
/* XTS decryption on raw arrays (no reference counterpart): dk1, rk2 [W*32][L] and out [sum len][8][L] (units in
 * order) follow `mem`; the units and their data are host pointers.  Units with equal tweaks share one T.  Calls
 * above TAE_CTR_CHUNK_BLOCKS blocks run in consecutive chunks with the tweaks resident */
int tae_aesx_xts_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *dk1, const uint64_t *rk2,
                                 const tae_xts_unit *units, size_t n_units, int rounds, uint64_t *out, int mem);
/* XTS decryption on handles (no reference counterpart): dk1, ek2 [W*32], out[sum len * 8].  An output bit carries
 * the ids of the tweak bits in its row, so XORing outputs that share tweak bits is TAE_E_INDEP */
int tae_aesx_xts_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *dk1, const tae_bit *const *ek2,
                             const tae_xts_unit *units, size_t n_units, int rounds, tae_bit **out);

/* ---- Multi-key batches: key expansion, cipher, CTR and CBC across AES keys -----------
 * The reference encrypts under one AES key and has no counterpart of these functions.  One FHE key, many AES
 * keys: a key table is n_keys expanded keys (or decryption keys) of one key size, contiguous as
 * [n_keys][W*32][L] with W = 44 / 52 / 60 and L = tae_bit_len.  Slot s is, bit for bit, an expanded key in the
 * layout of tae_aesx_*, and may be passed to any tae_aesx_* call as it is.  A slot that no block or stream of a
 * call refers to is not read, so a table may hold stale slots.  Bootstraps are per ciphertext, so the bits of
 * different keys share their launches, and every output word equals the one the tae_aesx_* call with that
 * slot's key gives.  Scope of tae_aesx_*: TAE_PARAMS_SQRD_LVL_* (gal-mul driver), key_bits 128 / 192 / 256;
 * every other model is TAE_E_PARAM, as are other key_bits and `rounds` outside 1..=Nr.  A slot index outside
 * 0..n_keys-1 (so any work with n_keys == 0), a counter range that wraps and a CBC len % 16 != 0 are
 * TAE_E_ARG.  n_blocks == 0, n_streams == 0 and, for the two key calls, n_keys == 0 are TAE_OK and write
 * nothing; a stream with len == 0 contributes nothing.  key_of_block, the stream arrays and `data` are host
 * pointers under either `mem`.  The noise schedule is the single-key one (no ciphertexts of different keys
 * meet), validated statically before any device work. */
/* one counter-mode stream: len bytes under slot `key`, counter blocks iv || be64(first_counter + i) */
typedef struct {
    int32_t key;
    uint8_t iv[8];
    uint64_t first_counter;
    const uint8_t *data; /* len AES-CTR ciphertext bytes, or NULL for the keystream */
    size_t len;
} tae_ctr_stream;
/* one CBC stream: len bytes (whole blocks) of ciphertext under slot `key` */
typedef struct {
    int32_t key;
    uint8_t iv[16];
    const uint8_t *data;
    size_t len;
} tae_cbc_stream;
/* batched FIPS-197 5.2 key expansion (no reference counterpart): fresh keys [n_keys][key_bits][L] -> table
 * [n_keys][W*32][L]; word i of all keys is bootstrapped together, so the chain of dependent bootstraps is that
 * of one key (50 / 54 / 65) whatever n_keys is */
int tae_aesm_key_schedule_raw(const tae_context *ctx, int key_bits, const uint64_t *keys, size_t n_keys, uint64_t *table,
                              int mem);
/* batched FIPS-197 5.3.5 decryption keys (no reference counterpart): table -> dtable, both [n_keys][W*32][L];
 * dtable must not be table */
int tae_aesm_decrypt_key_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys, uint64_t *dtable,
                             int mem);
/* FIPS-197 5.1 cipher, block i under slot key_of_block[i] (host int32 array; no reference counterpart): blocks /
 * out [n_blocks][128][L] */
int tae_aesm_encrypt_blocks_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                                const int32_t *key_of_block, const uint64_t *blocks, size_t n_blocks, int rounds,
                                uint64_t *out, int mem);
/* FIPS-197 5.3 inverse cipher, block i under slot key_of_block[i] of a table of decryption keys (no reference
 * counterpart) */
int tae_aesm_decrypt_blocks_raw(const tae_context *ctx, int key_bits, const uint64_t *dtable, size_t n_keys,
                                const int32_t *key_of_block, const uint64_t *blocks, size_t n_blocks, int rounds,
                                uint64_t *out, int mem);
/* number of round-1 SBOX groups of a set of streams (host only, no context; no reference counterpart): the
 * distinct (key, byte position, byte value) triples of their counter blocks.  Streams of one slot share groups,
 * streams of different slots share none.  A negative slot or a wrapping range is TAE_E_ARG */
int tae_aesm_ctr_plan(const tae_ctr_stream *streams, size_t n_streams, size_t *round1_groups);
/* tae_aesx_ctr_transcipher_raw for several streams (no reference counterpart): out = the streams' bytes
 * concatenated in stream order, [sum len][8][L]; data == NULL gives that stream's keystream.  Calls above
 * TAE_CTR_CHUNK_BLOCKS blocks in total run in consecutive chunks, a boundary may fall inside a stream, and the
 * result does not depend on the chunk size */
int tae_aesm_ctr_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                                 const tae_ctr_stream *streams, size_t n_streams, int rounds, uint64_t *out, int mem);
/* tae_aesx_cbc_transcipher_raw for several streams (no reference counterpart): out [sum len][8][L] in stream
 * order, each stream chained from its own iv */
int tae_aesm_cbc_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *dtable, size_t n_keys,
                                 const tae_cbc_stream *streams, size_t n_streams, int rounds, uint64_t *out, int mem);
/* batched key expansion on handles (no reference counterpart): keys[n_keys*key_bits] -> table[n_keys*W*32], the
 * bookkeeping of tae_aesx_key_schedule applied key by key */
int tae_aesm_key_schedule(const tae_context *ctx, int key_bits, const tae_bit *const *keys /*[n_keys*key_bits]*/,
                          size_t n_keys, tae_bit **table /*[n_keys*W*32]*/);
/* multi-stream CTR on handles (no reference counterpart): out[sum len * 8], the bookkeeping of
 * tae_aesx_ctr_transcipher applied stream by stream; handles of unreferenced slots are not read */
int tae_aesm_ctr_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *table, size_t n_keys,
                             const tae_ctr_stream *streams, size_t n_streams, int rounds, tae_bit **out);
/* multi-stream CBC on handles (no reference counterpart): out[sum len * 8], the bookkeeping of
 * tae_aesx_cbc_transcipher applied stream by stream */
int tae_aesm_cbc_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *dtable, size_t n_keys,
                             const tae_cbc_stream *streams, size_t n_streams, int rounds, tae_bit **out);

/* ---- AES-CCM decryption of public frames (RFC 3610 / NIST SP 800-38C) ------------------
 * The reference has no CCM and no counterpart of these functions.  The server holds the expanded key under FHE and
 * the frame in the clear: a nonce of 7..13 bytes (L = 15 - nonce_len), associated data, and `data` = the
 * encrypted payload followed by the tag_len-byte encrypted tag U.  With S_i = E(A_i), A_i = (L-1) || nonce || be_L(i),
 * the payload is data ^ S_1 S_2 .., the CBC-MAC X runs over B_0 || encoded AAD || zero-padded payload through the
 * forward cipher, and the frame is authentic iff the first tag_len bytes of X ^ S_0 ^ U are zero.  The server can
 * see neither: it returns the payload bits and those 8 tag_len tag-difference bits under FHE, and the client
 * decrypts both and accepts the payload iff every difference bit is 0.  There is no verdict bit.
 * Every A_i and B_0 goes through the cipher as one batch of public blocks; the chain then takes one cipher call per
 * MAC block, over all the frames of the call that still have one.  A payload bit has noise^2 = 8 + 1, a
 * tag-difference bit 16 (it holds no key bit), the round 0 of a chain step 8 + 1 + 1 at a public byte and
 * 8 + 8 + 1 at a payload byte.  Scope: TAE_PARAMS_SQRD_LVL_* (gal-mul driver), key_bits 128 / 192 / 256, decryption,
 * whole frames; every other model is TAE_E_PARAM.  `rounds` applies to every cipher call and must be 2..=Nr.
 * TAE_E_PARAM before any device work: a nonce outside 7..13 bytes, a tag_len outside 4, 6 .. 16, aad_len >= 0xFF00
 * (only the two-byte AAD length form is supported), a payload length that does not fit L bytes, len < tag_len,
 * rounds < 2.  A slot outside 0..n_keys-1 and null arrays are TAE_E_ARG.  The stream arrays and their bytes are
 * host pointers under either `mem`. */
/* one frame under slot `key` of a key table */
typedef struct {
    int32_t key;
    const uint8_t *nonce;
    size_t nonce_len;
    const uint8_t *aad; /* may be NULL when aad_len == 0 */
    size_t aad_len;
    const uint8_t *data; /* payload ciphertext || encrypted tag */
    size_t len;          /* >= tag_len */
} tae_ccm_stream;
/* the blocks of a frame (host only, no context; no reference counterpart): n_ctr = 1 + ceil(payload_len / 16)
 * counter blocks A_0 .., n_mac MAC blocks B_0 ..; each of the three arrays may be NULL (a first call for the
 * counts) or holds ctr_blocks [n_ctr][16], mac_blocks [n_mac][16] (0 where a payload byte goes) and mac_src
 * [n_mac][16] (-1: the byte is public, else the index of the payload byte) */
int tae_aesx_ccm_format(const uint8_t *nonce, size_t nonce_len, int tag_len, const uint8_t *aad, size_t aad_len,
                        size_t payload_len, size_t *n_ctr, size_t *n_mac, uint8_t *ctr_blocks, uint8_t *mac_blocks,
                        int64_t *mac_src);
/* noise bookkeeping of CCM decryption for a fresh key (no reference counterpart; no GPU): the key expansion, then a
 * frame with public, payload and padded MAC blocks.  TAE_OK, TAE_E_NOISE or TAE_E_INDEP; TAE_E_PARAM for other
 * models than the 1-bit one and for rounds outside 2..=Nr */
int tae_aesx_ccm_noise_schedule_check(int param_set, int key_bits, int rounds);
/* the forward cipher over arbitrary public 16-byte blocks (no reference counterpart): blocks [n_blocks][16] and
 * key_of_block are host pointers, out [n_blocks][128][L]; every word equals tae_aesm_encrypt_blocks_raw on trivial
 * encryptions of the blocks, and round 1 runs once per distinct (slot, byte position, byte value).  Serves CCM's
 * A_i and B_0, GCM-style iv12 || be32 counters and CFB decryption */
int tae_aesm_pub_keystream_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                               const int32_t *key_of_block, const uint8_t *blocks, size_t n_blocks, int rounds,
                               uint64_t *out, int mem);
/* CCM decryption of several frames (no reference counterpart): out_plain [sum (len - tag_len)][8][L], frames in
 * order (may be NULL when no frame has a payload); out_tag_diff [n_streams][8 tag_len][L] */
int tae_aesm_ccm_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                                 const tae_ccm_stream *streams, size_t n_streams, int tag_len, int rounds,
                                 uint64_t *out_plain, uint64_t *out_tag_diff, int mem);
/* the same on handles (no reference counterpart): out_plain[sum (len - tag_len) * 8], out_tag_diff[n_streams * 8
 * tag_len]; XORing two tag-difference bits of a frame, or one with a payload bit of another position, is legal */
int tae_aesm_ccm_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *table, size_t n_keys,
                             const tae_ccm_stream *streams, size_t n_streams, int tag_len, int rounds,
                             tae_bit **out_plain, tae_bit **out_tag_diff);
/* one frame under one expanded key rk [W*32][L] (no reference counterpart) */
int tae_aesx_ccm_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint8_t *nonce,
                                 size_t nonce_len, const uint8_t *aad, size_t aad_len, const uint8_t *data, size_t len,
                                 int tag_len, int rounds, uint64_t *out_plain, uint64_t *out_tag_diff, int mem);
/* one frame on handles (no reference counterpart): expanded_key [W*32] */
int tae_aesx_ccm_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                             const uint8_t *nonce, size_t nonce_len, const uint8_t *aad, size_t aad_len,
                             const uint8_t *data, size_t len, int tag_len, int rounds, tae_bit **out_plain,
                             tae_bit **out_tag_diff);

/* ---- AES-GCM decryption of public frames (NIST SP 800-38D) ------------------------------
 * The reference has no GCM and no counterpart of these functions.  The server holds the expanded key under FHE and
 * the frame in the clear: a 12-byte IV, associated data, and `data` = the ciphertext followed by the tag_len-byte
 * received tag.  With H = E(0^128) and J0 = iv || 00000001, payload block i is C_i ^ E(iv || be32(2 + i)) and the
 * frame is authentic iff the first tag_len bytes of E(J0) ^ GHASH_H(aad, C) ^ tag are zero.  The hashed blocks
 * X_1 .. X_m (padded AAD, padded ciphertext, the length block) are public, so GHASH = sum_i X_i H^(m+1-i) is a set
 * of LWE row sums over the key's power table H^1 .. H^n, which tae_aesx_ghash_key makes once per key: an even power
 * is a square (row sums and a refresh), an odd one a product of two encrypted elements (1024 nibble pairs through
 * one 8 -> 7 circuit bootstrap, chunk sums, a refresh, the reduction, a refresh).  The server returns the payload
 * bits and the 8 tag_len tag-difference bits under FHE; the client decrypts both and accepts the payload iff every
 * difference bit is 0.  There is no verdict bit.  A table bit has noise^2 = 1, a payload bit 8 + 1, a
 * tag-difference bit the number of refreshed chunks of its row (1 for up to 55 sources, one more per 64 beyond);
 * it holds no key bit.  Scope: TAE_PARAMS_SQRD_LVL_* (gal-mul driver), key_bits 128 / 192 / 256, decryption,
 * several frames under one key per call; every other model is TAE_E_PARAM.  `rounds` applies to every cipher call.
 * TAE_E_PARAM before any device work: an IV that is not 12 bytes (other lengths need GHASH over the IV), a tag_len
 * outside 4, 8, 12 .. 16, len < tag_len, rounds < 2 in the transcipher calls, n_powers outside 1..64 in tae_aesx_ghash_key*, a frame with
 * more hashed blocks than n_powers.  TAE_E_NOISE before any device work: a row that needs more than 64 chunks
 * (roughly m > 55).  Null arrays are TAE_E_ARG.  The frame arrays and their bytes are host pointers under either
 * `mem`. */
typedef struct {
    const uint8_t *iv;
    size_t iv_len;      /* 12 */
    const uint8_t *aad; /* may be NULL when aad_len == 0 */
    size_t aad_len;
    const uint8_t *data; /* ciphertext || received tag */
    size_t len;          /* >= tag_len */
} tae_gcm_frame;
/* the blocks of a frame (host only, no context): n_pub = 2 + ceil(data_len / 16) public cipher inputs 0^128, J0,
 * iv || be32(2 + i) (the low 32 bits wrap modulo 2^32), n_hashed = m hashed blocks X_1 .. X_m; each array may be NULL
 * (a first call for the counts) or holds pub_blocks [n_pub][16] and hashed_blocks [n_hashed][16].  `data` is the
 * ciphertext alone */
int tae_aesx_gcm_format(const uint8_t *iv, size_t iv_len, const uint8_t *aad, size_t aad_len, const uint8_t *data,
                        size_t data_len, int tag_len, size_t *n_pub, size_t *n_hashed, uint8_t *pub_blocks,
                        uint8_t *hashed_blocks);
/* the tag rows of a frame against a table of n_powers (host only): row_sources[r] table bits and row_chunks[r]
 * refreshed chunks for r < 8 tag_len, written before the refusals TAE_E_PARAM (m > n_powers) and TAE_E_NOISE */
int tae_aesx_gcm_tag_rows(const uint8_t *iv, size_t iv_len, const uint8_t *aad, size_t aad_len, const uint8_t *data,
                          size_t data_len, int tag_len, size_t n_powers, int32_t *row_sources, int32_t *row_chunks);
/* noise bookkeeping for a fresh key (no GPU): the key expansion, the power table, then a frame of aad_len + data_len
 * dense bytes with a 16-byte tag.  TAE_OK, TAE_E_NOISE, TAE_E_INDEP or TAE_E_PARAM */
int tae_aesx_gcm_noise_schedule_check(int param_set, int key_bits, int rounds, int n_powers, size_t aad_len,
                                      size_t data_len);
/* the power table: rk [W*32][L] -> hk [n_powers][128][L], power k at block k - 1, coefficient i at ciphertext i */
int tae_aesx_ghash_key_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, int n_powers, int rounds,
                           uint64_t *hk, int mem);
/* the same on handles: hk[n_powers * 128], every bit at noise^2 = 1 with a fresh id */
int tae_aesx_ghash_key(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key, int n_powers, int rounds,
                       tae_bit **hk);
/* GCM decryption of n_frames frames under one key: out_plain [sum (len - tag_len)][8][L], frames in order (may be
 * NULL when no frame has a payload); out_tag_diff [n_frames][8 tag_len][L] */
int tae_aesx_gcm_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint64_t *hk,
                                 size_t n_powers, const tae_gcm_frame *frames, size_t n_frames, int tag_len, int rounds,
                                 uint64_t *out_plain, uint64_t *out_tag_diff, int mem);
/* the same on handles: out_plain[sum (len - tag_len) * 8], out_tag_diff[n_frames * 8 tag_len]; XORing two
 * tag-difference bits, or one with a payload bit, is legal */
int tae_aesx_gcm_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                             const tae_bit *const *hk, size_t n_powers, const tae_gcm_frame *frames, size_t n_frames,
                             int tag_len, int rounds, tae_bit **out_plain, tae_bit **out_tag_diff);
/* ---- GCM over key tables ---------------------------------------------------------------
 * The two calls above for many AES keys under one FHE key: `table` is a key table [n_keys][W*32][L] as in the
 * multi-key batches, `htable` the power tables of its slots [n_keys][n_powers][128][L], and every frame names its slot.
 * tae_aesm_ghash_key* makes all power tables in the launch sequence of one (a generation's squares and products of all
 * keys share their launches, the products in batches of TAE_GCM_SEG_BATCH); tae_aesm_gcm_transcipher* runs the frames of
 * all slots through one public pass, one chunk-sum launch that reads `htable` in place, one refresh and one difference
 * launch.  Slot s of the result, and every frame's words, levels and ids, equal the single-key call on table[s] /
 * htable[s].  Scope and refusals of the single-key calls; one key size and one tag_len per call.  A slot outside
 * 0..n_keys-1 and null arrays are TAE_E_ARG.  The frames are validated before the context is looked at.  A slot no
 * frame names is not read, in either table; with TAE_MEM_HOST only the named slots are uploaded. */
/* one frame under slot `key` of both tables */
typedef struct {
    int32_t key;
    const uint8_t *iv;
    size_t iv_len;      /* 12 */
    const uint8_t *aad; /* may be NULL when aad_len == 0 */
    size_t aad_len;
    const uint8_t *data; /* ciphertext || received tag */
    size_t len;          /* >= tag_len */
} tae_gcm_stream;
/* table [n_keys][W*32][L] -> htable [n_keys][n_powers][128][L] */
int tae_aesm_ghash_key_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys, int n_powers,
                           int rounds, uint64_t *htable, int mem);
/* the same on handles: table[n_keys * W*32] -> htable[n_keys * n_powers * 128], every bit at noise^2 = 1 with a
 * fresh id */
int tae_aesm_ghash_key(const tae_context *ctx, int key_bits, const tae_bit *const *table, size_t n_keys, int n_powers,
                       int rounds, tae_bit **htable);
/* out_plain [sum (len - tag_len)][8][L], frames in order (may be NULL when no frame has a payload); out_tag_diff
 * [n_streams][8 tag_len][L] */
int tae_aesm_gcm_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                                 const uint64_t *htable, size_t n_powers, const tae_gcm_stream *streams, size_t n_streams,
                                 int tag_len, int rounds, uint64_t *out_plain, uint64_t *out_tag_diff, int mem);
/* the same on handles; the entries of slots no frame names may be NULL in both tables */
int tae_aesm_gcm_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *table, size_t n_keys,
                             const tae_bit *const *htable, size_t n_powers, const tae_gcm_stream *streams,
                             size_t n_streams, int tag_len, int rounds, tae_bit **out_plain, tae_bit **out_tag_diff);
/* ---- frames beyond one table: segmented GHASH ------------------------------------------
 * tae_aesx_gcm_transcipher* stops at about 55 hashed blocks.  These calls split GHASH into C = ceil(m / seg) segments
 * of seg hashed blocks.  With e = m + 1 - i the exponent of X_i, c = (e - 1) / seg and k = (e - 1) % seg + 1:
 *   GHASH = S_0 + sum_{c >= 1} S_c H^(seg c),   S_c = sum_k X_(c,k) H^k
 * so every segment is row sums over the table's first seg powers, and each inner segment (c >= 1) is lifted by one
 * product with a stride power H^(seg c).  The stride key holds H^(seg j) at entry j - 1 and is made once per key and
 * seg from the power table; a frame takes up to (n_strides + 1) seg hashed blocks.  Inputs and outputs are those of
 * tae_aesx_gcm_transcipher*; a frame of at most seg hashed blocks gives the same words as that call.  Levels: an
 * inner chunk sums at most 64 table bits, an inner row its refreshed chunks (at most 64) and is refreshed to 1, the
 * product bits are 1 with fresh ids and enter the final rows like table bits; a tag-difference bit is the number of
 * refreshed chunks of its final row.  TAE_E_PARAM before any device work, beside the conditions above: seg outside
 * 1 .. min(n_powers, 64), n_strides outside 1 .. 64, a frame with C - 1 > n_strides.  TAE_E_NOISE before any device work: an
 * inner or a final row of more than 64 chunks.  A hashed block puts at most 128 sources into a row, so seg <= 31 is
 * never refused for noise (31 * 128 + 64 <= 55 + 63 * 64); longer segments depend on the data (about 50 chunks a row
 * at seg = 48 on random blocks). */
/* the rows of a frame (host only): row_sources / row_chunks [C][128], C = ceil(n_hashed / seg).  Segment 0 holds the
 * final rows r < 8 tag_len (table bits and one bit per product; the rest of its 128 entries is 0), segment c >= 1 the
 * 128 inner rows of S_c.  For seg >= 1 they are written before the refusals */
int tae_aesx_gcm_long_rows(const uint8_t *iv, size_t iv_len, const uint8_t *aad, size_t aad_len, const uint8_t *data,
                           size_t data_len, int tag_len, size_t n_powers, size_t seg, size_t n_strides,
                           int32_t *row_sources, int32_t *row_chunks);
/* noise bookkeeping for a fresh key (no GPU): the key expansion, the power table, the stride key, then a frame of
 * aad_len + data_len dense bytes with a 16-byte tag */
int tae_aesx_gcm_long_noise_schedule_check(int param_set, int key_bits, int rounds, int n_powers, size_t seg,
                                           int n_strides, size_t aad_len, size_t data_len);
/* the stride key: hk [n_powers][128][L] -> sk [n_strides][128][L], entry 0 a copy of hk's block seg - 1, an even
 * stride a square, an odd one a product with entry 0 */
int tae_aesx_ghash_stride_key_raw(const tae_context *ctx, const uint64_t *hk, size_t n_powers, size_t seg, int n_strides,
                                  uint64_t *sk, int mem);
/* the same on handles: sk[n_strides * 128]; entry 0 clones the table's bits and shares their ids, every later bit is
 * noise^2 = 1 with a fresh id */
int tae_aesx_ghash_stride_key(const tae_context *ctx, const tae_bit *const *hk, size_t n_powers, size_t seg, int n_strides,
                              tae_bit **sk);
int tae_aesx_gcm_long_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint64_t *hk,
                                      size_t n_powers, const uint64_t *sk, size_t n_strides, size_t seg,
                                      const tae_gcm_frame *frames, size_t n_frames, int tag_len, int rounds,
                                      uint64_t *out_plain, uint64_t *out_tag_diff, int mem);
int tae_aesx_gcm_long_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                                  const tae_bit *const *hk, size_t n_powers, const tae_bit *const *sk, size_t n_strides,
                                  size_t seg, const tae_gcm_frame *frames, size_t n_frames, int tag_len, int rounds,
                                  tae_bit **out_plain, tae_bit **out_tag_diff);
/* stage entries for tests: the squares, and the products a_c b_c, of `count` field elements [count][128][L]
 * (coefficient i of GCM's bit-reflected field at ciphertext i), every output bit refreshed to noise^2 = 1 */
int tae_stage_gf128_square(const tae_context *ctx, const uint64_t *in, size_t count, uint64_t *out, int mem);
int tae_stage_gf128_product(const tae_context *ctx, const uint64_t *a, const uint64_t *b, size_t count, uint64_t *out,
                            int mem);

/* ---- AEAD open: a tag verdict bit and the verdict-gated payload (no counterpart in the reference) ----
 * The CCM and GCM calls above return the payload bits [sum payload_lens][8][L], frames in order, and the
 * tag-difference bits [n_frames][8 tag_len][L], and leave the verdict to the client.  These calls join the two on the
 * server: ok [n_frames][L] encrypts 1 iff every difference bit of the frame is 0 (levels of "OR of 8" circuit
 * bootstraps, the last one "NOR of 8": 128 -> 16 -> 2 -> 1), and out_plain is the payload where ok = 1 and all zeros
 * where ok = 0 (one 9 -> 8 circuit bootstrap per byte: its 8 bits and the frame's verdict).  One tag_len per call, any
 * length CCM or GCM accepts (4 .. 16 even, 13, 15); a frame of length 0 still gets its verdict.
 * 1-bit WoP-PBS parameter sets only: the 8-bit model and shortint_1bit are TAE_E_PARAM, as is another tag_len; both
 * come before any device work and leave the stage times untouched.  n_frames == 0 is a no-op.
 * Noise: every input of a bootstrap must be at or below the cap of the parameter set (TAE_E_NOISE); verdict bits come
 * out at noise^2 = 8 and gated payload bits at 9, with fresh ids and no key bit.  The raw forms replay this for inputs
 * at the cap; the handle form for its inputs' levels. */
/* The plan alone, no GPU: *levels (2 or 3), verdict_groups [*levels] (room for 3: the groups per frame of every
 * level) and *gate_groups = sum payload_lens */
int tae_aead_open_plan(int tag_len, const size_t *payload_lens, size_t n_frames, int *levels, size_t *verdict_groups,
                       size_t *gate_groups);
/* the schedule of one frame of one byte with payload bits at plain_level and difference bits at diff_level */
int tae_aead_open_noise_schedule_check(int param_set, int tag_len, uint64_t plain_level, uint64_t diff_level);
int tae_aead_verdict_raw(const tae_context *ctx, const uint64_t *tag_diff, size_t n_frames, int tag_len, uint64_t *ok,
                         int mem);
/* payload_lens is a host array in either memory kind; out_plain is not plain */
int tae_aead_open_raw(const tae_context *ctx, const uint64_t *plain, const size_t *payload_lens, const uint64_t *tag_diff,
                      size_t n_frames, int tag_len, uint64_t *out_plain, uint64_t *out_ok, int mem);
/* plain [sum payload_lens * 8] and tag_diff [n_frames * 8 tag_len] handles -> out_plain [sum payload_lens * 8],
 * out_ok [n_frames] */
int tae_aead_open(const tae_context *ctx, const tae_bit *const *plain, const size_t *payload_lens,
                  const tae_bit *const *tag_diff, size_t n_frames, int tag_len, tae_bit **out_plain, tae_bit **out_ok);

/* ---- Aes128Encrypt for the fhe_sbox_pbs driver (src/aes_128/fhe/fhe_sbox_pbs.rs:22-171) ------------
 * ShortintWoppbs1BitSboxPbsAesEncrypt on the 1-bit model (fhe_impls/shortint_woppbs_1bit.rs:47-81:
 * SubBytes = one 8 -> 8 circuit bootstrap per byte, MixColumns = gf_256_mul by BitCt XORs) and
 * ShortintWoppbs8BitSboxPbsAesEncrypt on the 8-bit model (same as tae_aes_* there).  On the 1-bit model
 * every MixColumns breaks the BitCt noise rules, so rounds >= 2 return TAE_E_INDEP before any device work,
 * where the reference panics "noise components not independent" (its test_light / test_full of this
 * combination are #[ignore]d, :160-176); rounds == 1 and the key schedule run batched on the device. */
int tae_aes_sbox_pbs_encrypt_blocks(const tae_context *ctx, const tae_bit *const *expanded_key,
                                    const tae_bit *const *blocks, size_t n_blocks, int rounds, tae_bit **out);
/* fhe_sbox_pbs::key_schedule (:123-171): key[128] bits -> expanded[44*32] bits */
int tae_aes_sbox_pbs_key_schedule(const tae_context *ctx, const tae_bit *const *key, tae_bit **expanded);
int tae_aes_sbox_pbs_encrypt_blocks_raw(const tae_context *ctx, const uint64_t *rk, const uint64_t *blocks,
                                        size_t n_blocks, int rounds, uint64_t *out, int mem);
int tae_aes_sbox_pbs_key_schedule_raw(const tae_context *ctx, const uint64_t *key, uint64_t *expanded, int mem);

/* Static check of a driver's round-function noise schedule for fresh inputs (no context, no device):
 * TAE_OK, or the status the reference's panic maps to (TAE_E_INDEP / TAE_E_NOISE). */
#define TAE_DRIVER_GAL_MUL 0  /* fhe_sbox_gal_mul_pbs */
#define TAE_DRIVER_SBOX_PBS 1 /* fhe_sbox_pbs */
int tae_aes_noise_schedule_check(int param_set, int driver, int rounds);

/* ---- packed ciphertext I/O (no reference counterpart) -------------------------
 * A bit crosses the boundary as one coefficient of a GLWE instead of one big-key LWE: 40 bytes instead of 16392
 * (20 in the 32-bit wire form).  TAE_PARAMS_SQRD_LVL_64 only: every other parameter set is TAE_E_PARAM.
 * Format: `count` bits occupy G = ceil(count / N) GLWEs [G][(k+1)N] u64, mask polynomials first, body last;
 * bit j sits at coefficient j % N of GLWE j / N, encoded bit << 63; unused coefficients of the last GLWE carry
 * zero (plus noise).  count == 0 and null pointers are TAE_E_ARG before any device work.
 *
 * Uploads: the client encrypts 512 bits per GLWE (tae_encrypt_packed_raw) and the server sample-extracts them
 * into big-key bits (tae_unpack_bits*), exactly: the big LWE key is the flattened GLWE key, no noise is added,
 * and the GLWE noise is below a fresh bit's, so every extracted bit is a noise-level-1 bit.
 * Results: the server packs any bits with the last private functional keyswitch key (plaintext polynomial -1)
 * and a rotate-and-sum (tae_pack_bits*), the client decrypts the GLWEs (tae_decrypt_packed_raw).
 * Server-packed GLWEs are terminal: they are for the client or for storage, the noise bookkeeping has no rule
 * for them, and unpacking is defined for client-made GLWEs only. */
/* G and G (k+1) N for `count` bits (either output may be NULL) */
int tae_packed_len(int param_set, size_t count, size_t *glwes, size_t *words);
/* bits[count] (0 / 1) -> glwes [G][(k+1)N]; GLWE g is encryption #start_index + g of the packed stream (its own
 * index space: it shares no mask with the per-bit encryptions of the same index), TAE_INDEX_AUTO reserves G
 * fresh indices from the key's counter */
int tae_encrypt_packed_raw(const tae_client_key *ck, const uint8_t *bits, size_t count, uint64_t start_index,
                           uint64_t *glwes);
int tae_decrypt_packed_raw(const tae_client_key *ck, const uint64_t *glwes, size_t count, uint8_t *bits);
/* the 32-bit wire form: narrow[i] = (wide[i] + 2^31) >> 32, and back wide[i] = narrow[i] << 32 (host arrays).
 * Widen before tae_decrypt_packed_raw or tae_unpack_bits*; the rounding adds an error below 2^31 per word */
int tae_packed_narrow(const uint64_t *wide, size_t words, uint32_t *narrow);
int tae_packed_widen(const uint32_t *narrow, size_t words, uint64_t *wide);
/* glwes [G][(k+1)N] -> bits [count][K+1]; without a GPU TAE_E_NODEV */
int tae_unpack_bits_raw(const tae_context *ctx, const uint64_t *glwes, size_t count, uint64_t *bits, int mem);
/* bits [count][K+1] -> glwes [G][(k+1)N]; without a GPU TAE_E_NODEV */
int tae_pack_bits_raw(const tae_context *ctx, const uint64_t *bits, size_t count, uint64_t *glwes, int mem);
/* handles: glwes is a host array; every bit comes out at noise level 1 with a fresh id */
int tae_unpack_bits(const tae_context *ctx, const uint64_t *glwes, size_t count, tae_bit **out /*[count]*/);
/* any valid bits, whatever their noise level; glwes is a host array */
int tae_pack_bits(const tae_context *ctx, const tae_bit *const *bits, size_t count, uint64_t *glwes);
/* ms of the keyswitch slice and the rotate-and-sum of the context's last tae_pack_bits* call (timing on);
 * the per-stage slots of tae_last_stage_times* keep the values of the last batched call */
int tae_last_pack_time(const tae_context *ctx, double *ms);

/* ---- stage entry points (raw arrays; parity tests and profiling) ---------------------------- */
/* the keyswitch of tae_pack_bits_raw before the sum: out [count][(k+1)N], row b the private functional
 * keyswitch of bit b with key k (coefficient 0 of its body carries the bit's phase) */
int tae_stage_pack_pfks(const tae_context *ctx, const uint64_t *bits, size_t count, uint64_t *out, int mem);
int tae_stage_keyswitch(const tae_context *ctx, const uint64_t *in, size_t count, uint64_t *out, int mem);
int tae_stage_pbs_shift_boolean(const tae_context *ctx, const uint64_t *small, size_t count, int level,
                                uint64_t *big, int mem);
int tae_stage_bootstrap(const tae_context *ctx, const uint64_t *small, size_t count,
                        const uint64_t *lut_glwe, uint64_t *big, int mem);
int tae_stage_pfks_ggsw(const tae_context *ctx, const uint64_t *big, size_t count, int level,
                        uint64_t *ggsw, int mem);
int tae_stage_ggsw_fourier(const tae_context *ctx, const uint64_t *ggsw, size_t count,
                           double *ggsw_f /*complex interleaved*/, int mem);
/* ggsw_f [groups][n_in] Fourier GGSWs (selector bits, MSB first), out [groups][n_out][K+1].  With
 * tree = max(0, n_in - log2 N), lut is [n_out][N << tree] words: 2^tree polynomials per output, chosen by the
 * first `tree` GGSWs through a CMux tree (one polynomial per output while n_in <= log2 N).  The length is the
 * same for TAE_MEM_HOST, where that many words are staged, and for a TAE_MEM_DEVICE pointer.  n_in < 1,
 * n_out < 1 or tree > 16 return TAE_E_ARG before any device work. */
int tae_stage_vertical_packing(const tae_context *ctx, const double *ggsw_f, size_t groups, int n_in,
                               const uint64_t *lut, int n_out, uint64_t *out, int mem);

/* ---- device utilities -------------------------------------------------------------------- */
int tae_synchronize(const tae_context *ctx);
/* TAE_MEM_DEVICE inputs are produced on `stream` (a hipStream_t of the context's device, e.g. torch's
 * current stream); NULL restores the device-wide synchronize.  Not thread-safe against calls in flight. */
int tae_set_caller_stream(tae_context *ctx, void *stream);
/* 0 off; 1 per-stage HIP-event times of each batched call; 2 the same plus in-kernel clock stamps of the
 * throughput blind-rotation launches (a diagnostic mode: every stamped launch is read back synchronously) */
int tae_set_timing(const tae_context *ctx, int on);
/* per-stage ms of the last batched call: [keyswitch, pbs, pfks, ggsw_fft, vp] */
int tae_last_stage_times(const tae_context *ctx, float *ms5);
/* [keyswitch, pbs, pfks, ggsw_fft, vp, extract_bits, linear] ms + the CBS-level PBS launch count */
int tae_last_stage_times_v2(const tae_context *ctx, float *ms8);
/* v2's eight values, then the ms and the ciphertext count of the throughput blind-rotation kernel's
 * own launches (br512x4, without the small-batch remainder) -- the roofline's launch duration */
int tae_last_stage_times_v3(const tae_context *ctx, double *v10);
/* v3's ten values, then (timing mode 2) the effective shader clock in GHz of the throughput blind-rotation
 * launches (median over each launch's workgroups of shader cycles / 100 MHz reference ticks, averaged over
 * the launches; MI355X_MICROARCH.md "DVFS give-back") and the number of launches it averages (0: none) */
int tae_last_stage_times_v4(const tae_context *ctx, double *v12);
/* name of the kernel that the context's last private functional keyswitch launched, NUL-terminated into
 * name[cap]: "g6", "s16", "w32", "w16" (the K-layout int8 GEMMs, chosen by TAE_PFKS_GEMM at context creation),
 * "rows" (the row-limb GEMM of small batches), "u64" (the scalar kernel) or "none" */
int tae_last_pfks_kernel(const tae_context *ctx, char *name, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
