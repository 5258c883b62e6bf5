// Host-side mirror of the reference's model and AES traits, driving the device Engine.
//
// Reference (allanbrondum/tfhe-aes-2):
//   src/tfhe.rs:11-24                       ClientKeyT / ContextT
//   src/tfhe/shortint_woppbs_1bit.rs:26-151  BitCt, NoiseLevelWithComponents, BitXorAssign
//   src/tfhe/shortint_woppbs_1bit.rs:165-336 FheContext (ct ids, generate_lookup_table,
//                                            circuit_bootstrap)
//   src/aes_128/fhe/fhe_impls/shortint_woppbs_1bit.rs:17-151
//                                            ByteT impls + ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
//   src/aes_128/fhe/fhe_sbox_gal_mul_pbs.rs:27-191 encrypt_block_for_rounds, key_schedule
//   src/aes_128/fhe/fhe_sbox_pbs.rs:22-171   the same for the fhe_sbox_pbs driver
// The ciphertext arithmetic runs in the Engine (HIP); this layer keeps the reference's noise
// bookkeeping (noise^2 level + independent component ids) on the host, per ciphertext.
#pragma once
#include <atomic>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "client.hpp"
#include "engine.hpp"

namespace tae {

// Reference panics become status codes.
struct ModelError {
    int code;  // TAE_E_NOISE / TAE_E_INDEP / TAE_E_PARAM / TAE_E_ARG
    std::string msg;
};

// NoiseLevelWithComponents (shortint_woppbs_1bit.rs:34-78)
struct NoiseLevel {
    uint64_t noise_level_squared = 0;
    std::vector<uint64_t> components;  // sorted CiphertextIds

    static NoiseLevel with_noise_level(uint64_t nl, uint64_t id) { return {nl, {id}}; }
    static NoiseLevel trivial() { return {}; }
    // add_assign: asserts disjoint components, unions them, adds noise^2 and validates <= max
    void add_assign(const NoiseLevel &rhs, uint64_t max_noise_sq);
};

uint64_t next_ct_id();  // FheContext::next_ct_id (process-wide counter)

struct BitCt {
    std::vector<uint64_t> ct;  // [K+1]
    NoiseLevel noise;
    uint64_t max_noise_sq = 0;

    void xor_assign(const BitCt &rhs);  // BitXorAssign
};

enum class AesDriver { GalMul, SboxPbs };

struct Lut {  // WopbsLUTBase
    int input_bits = 0, output_bits = 0;
    size_t small_len = 0;
    std::vector<uint64_t> data;  // [output_bits][small_len]
};

class Context {  // FheContext
  public:
    Context(std::unique_ptr<Engine> engine) : engine_(std::move(engine)) {}
    const Params &params() const { return engine_->params(); }
    Engine &engine() { return *engine_; }
    std::mutex &mutex() { return mu_; }

    BitCt trivial(uint64_t bit) const;
    BitCt wrap(std::vector<uint64_t> ct, uint64_t noise_level_squared) const;  // BitCt::with_noise_level
    Lut generate_lookup_table(int input_bits, int output_bits, const uint64_t *f_values) const;
    std::vector<BitCt> circuit_bootstrap(const std::vector<const BitCt *> &bits, const Lut &lut);
    // batched raw circuit bootstrap (device or host arrays)
    void circuit_bootstrap_raw(const uint64_t *bits, size_t groups, int n_in, const Lut &lut, uint64_t *out,
                               bool device_mem);

    // Aes128Encrypt::encrypt_block_for_rounds over many blocks (noise bookkeeping per bit).  Driver
    // GalMul = fhe_sbox_gal_mul_pbs (ShortintWoppbs1BitSboxGalMulPbsAesEncrypt); SboxPbs = fhe_sbox_pbs
    // (ShortintWoppbs1BitSboxPbsAesEncrypt on the 1-bit model).  The 8-bit model has fhe_sbox_pbs only
    // (ShortintWoppbs8BitSboxPbsAesEncrypt) and ignores the flag.
    // key_bits (here and below) = 128 / 192 / 256, anything else is TAE_E_PARAM: the key has W = 44 / 52 / 60
    // words (another size is TAE_E_ARG) and rounds goes up to Nr = 10 / 12 / 14.  192 and 256 run on the 1-bit
    // model with the gal-mul driver only (TAE_E_PARAM elsewhere).
    std::vector<BitCt> aes_encrypt_blocks(const std::vector<const BitCt *> &expanded_key,
                                          const std::vector<const BitCt *> &blocks, size_t n_blocks, int rounds,
                                          AesDriver driver = AesDriver::GalMul, int key_bits = 128);
    // key_schedule: fhe_sbox_gal_mul_pbs (:134-164) or fhe_sbox_pbs (:123-171)
    std::vector<BitCt> aes_key_schedule(const std::vector<const BitCt *> &key, AesDriver driver = AesDriver::GalMul);
    // raw arrays, fresh inputs; static noise-schedule validation
    void aes_encrypt_blocks_raw(const uint64_t *rk, const uint64_t *blocks, size_t n_blocks, int rounds,
                                uint64_t *out, bool device_mem, AesDriver driver = AesDriver::GalMul, int key_bits = 128);
    // raw key schedule: key [128][bit_len] fresh bits -> [44*32][bit_len]
    void aes_key_schedule_raw(const uint64_t *key, uint64_t *expanded, bool device_mem,
                              AesDriver driver = AesDriver::GalMul);
    // FIPS-197 5.2 key expansion on the device (Engine::aes_key_expand), 1-bit model only: key [Nk*32] ->
    // [W*32].  Words below Nk are the key's bits; every later word leaves its identity bootstrap at noise^2 = 1
    // with fresh ids.  At 128 bits the words equal aes_key_schedule's.  The BitCt variant replays the
    // bookkeeping (aes_key_expand_noise_schedule) before any device work, the raw one for a fresh key.
    std::vector<BitCt> aes_key_expand(const std::vector<const BitCt *> &key, int key_bits);
    void aes_key_expand_raw(const uint64_t *key, uint64_t *expanded, bool device_mem, int key_bits);

    // ---- AES-128-CTR with public counters (main.rs:108-128): counter block i = iv || be64(first_counter + i)
    // is public, so no counter ciphertexts exist and round 1 is bootstrapped once per distinct (position,
    // byte) pair (ctr_plan.hpp).  Gal-mul driver on the 1-bit sets, fhe_sbox_pbs on the 8-bit set;
    // SHORTINT_1BIT is TAE_E_PARAM.  The noise schedule is validated statically for trivial blocks. ----
    // keystream blocks [n_blocks][128][bit_len]; rk / out host or device, iv host
    void aes_ctr_keystream_raw(const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter, size_t n_blocks,
                               int rounds, uint64_t *out, bool device_mem, int key_bits = 128);
    // data (host bytes, AES-CTR ciphertext) -> [len][8][bit_len] encryptions of the plaintext bits
    void aes_ctr_transcipher_raw(const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter, const uint8_t *data,
                                 size_t len, int rounds, uint64_t *out, bool device_mem, int key_bits = 128);
    // BitCt variant, [len*8] bits with the schedule's noise; with rounds == 1 outputs that share a round-1
    // group share its component id
    std::vector<BitCt> aes_ctr_transcipher(const std::vector<const BitCt *> &expanded_key, const uint8_t iv[8],
                                           uint64_t first_counter, const uint8_t *data, size_t len,
                                           int rounds = 10, int key_bits = 128);

    // ---- AES-128 inverse cipher, FIPS-197 5.3 (the reference has no decryption; aes_inv.hpp): InvSubBytes and
    // InvMixColumns' multiples {14,11,13,9} in one 8 -> 32 circuit bootstrap per byte, `rounds` bootstraps per
    // block.  1-bit WoP-PBS sets (gal-mul driver) only: every other model is TAE_E_PARAM. ----
    // decryption key [44*32]: words 0..3 / 40..43 unchanged, words 4r..4r+3 = InvMixColumns(rk[r]) with fresh
    // noise (noise^2 = 1, new ids)
    // (with key_bits: words 0..3 and 4 Nr .. 4 Nr + 3 unchanged, words 4 .. 4 Nr - 1 derived)
    std::vector<BitCt> aes_decrypt_key(const std::vector<const BitCt *> &expanded_key, int key_bits = 128);
    void aes_decrypt_key_raw(const uint64_t *rk, uint64_t *dk, bool device_mem, int key_bits = 128);
    // inverts aes_encrypt_blocks(rounds): round keys Nr (10), rounds-1 .. 1, 0.  Noise bookkeeping per bit
    std::vector<BitCt> aes_decrypt_blocks(const std::vector<const BitCt *> &dk, const std::vector<const BitCt *> &blocks,
                                          size_t n_blocks, int rounds, int key_bits = 128);
    // raw arrays; the schedule is validated statically for a derived key and fresh blocks
    void aes_decrypt_blocks_raw(const uint64_t *dk, const uint64_t *blocks, size_t n_blocks, int rounds, uint64_t *out,
                                bool device_mem, int key_bits = 128);
    // CBC with a public ciphertext: data (host bytes, len % 16 == 0 or TAE_E_ARG) -> [len][8][bit_len]
    // encryptions of P_i = Dec(C_i) ^ C_{i-1}, C_{-1} = iv; no input ciphertexts are made
    void aes_cbc_transcipher_raw(const uint64_t *dk, const uint8_t iv[16], const uint8_t *data, size_t len, int rounds,
                                 uint64_t *out, bool device_mem, int key_bits = 128);
    std::vector<BitCt> aes_cbc_transcipher(const std::vector<const BitCt *> &dk, const uint8_t iv[16],
                                           const uint8_t *data, size_t len, int rounds = 10, int key_bits = 128);

    // ---- XTS-AES decryption of a public ciphertext (IEEE 1619; aes_xts.hpp; the reference has no
    // XTS).  1-bit WoP-PBS sets, gal-mul driver, one key_bits for both keys (TAE_E_PARAM elsewhere).  Block j of a
    // data unit: P_j = Dec_K1(C_j ^ M_j) ^ M_j, M_j = alpha^j Enc_K2(tweak).  `rounds` applies to both ciphers. ----
    struct XtsUnitIn {
        uint8_t tweak[16];
        uint64_t first_block;  // data starts at this block of the unit
        const uint8_t *data;
        size_t len;  // a positive multiple of 16, or TAE_E_PARAM
    };
    // T = Enc_K2(tweak) after its identity bootstrap: rk2 [W*32], tweaks [n][16] host bytes -> [n][128][bit_len] at
    // noise^2 = 1.  Equal tweaks are computed once and come out as identical words
    void aes_xts_tweaks_raw(const uint64_t *rk2, const uint8_t *tweaks, size_t n, int rounds, uint64_t *out,
                            bool device_mem, int key_bits);
    // the mask stage alone: masks [nb][128][bit_len], block b = alpha^block_index[b] of tweak ciphertext
    // unit_of_block[b] (host arrays; a unit outside 0..n_units-1 is TAE_E_ARG).  No noise rule: a stage call
    void xts_masks_raw(const uint64_t *tweak_cts, size_t n_units, const int32_t *unit_of_block,
                       const uint64_t *block_index, size_t nb, uint64_t *masks, bool device_mem);
    // out [sum len][8][bit_len], units in order.  The schedule is validated statically for derived keys, at the
    // block index of the call with the largest row weight: TAE_E_NOISE before any device work
    void aes_xts_transcipher_raw(const uint64_t *dk1, const uint64_t *rk2, const std::vector<XtsUnitIn> &units,
                                 int rounds, uint64_t *out, bool device_mem, int key_bits);
    // BitCt variant: an output bit carries 8 + 1 + its row weight and the ids of the tweak bits in its row; units
    // with equal tweaks share their tweak bits
    std::vector<BitCt> aes_xts_transcipher(const std::vector<const BitCt *> &dk1, const std::vector<const BitCt *> &ek2,
                                           const std::vector<XtsUnitIn> &units, int rounds, int key_bits);

    // ---- multi-key batches (the reference has one key): a key table is n_keys expanded (or
    // decryption) keys of one size, [n_keys][W*32][bit_len], slot s an expanded key as above.  1-bit model, gal-mul
    // driver (TAE_E_PARAM elsewhere).  Slots, streams and public bytes are host arrays; a slot outside
    // 0..n_keys-1 is TAE_E_ARG, a slot nothing refers to is not read.  The noise schedule is the single-key one,
    // validated statically (raw) or per key / per stream (BitCt). ----
    struct CtrStreamIn {
        CtrStream s;
        const uint8_t *data;  // len bytes, or nullptr for the keystream
    };
    struct CbcStreamIn {
        int32_t slot;
        uint8_t iv[16];
        const uint8_t *data;
        size_t len;  // whole blocks, or TAE_E_ARG
    };
    using BitAt = std::function<const BitCt *(size_t)>;  // bit i of a handle array, read for referenced slots only
    // keys [n_keys][key_bits][bit_len] -> table
    void aes_key_expand_multi_raw(const uint64_t *keys, size_t n_keys, uint64_t *table, bool device_mem, int key_bits);
    std::vector<BitCt> aes_key_expand_multi(const std::vector<const BitCt *> &keys, size_t n_keys, int key_bits);
    void aes_decrypt_key_multi_raw(const uint64_t *table, size_t n_keys, uint64_t *dtable, bool device_mem, int key_bits);
    // block i under slot key_of[i]; inverse: the table holds decryption keys
    void aes_blocks_multi_raw(bool inverse, const uint64_t *table, size_t n_keys, const int32_t *key_of,
                              const uint64_t *blocks, size_t n_blocks, int rounds, uint64_t *out, bool device_mem,
                              int key_bits);
    // out = the streams' bytes concatenated in stream order [sum len][8][bit_len]
    void aes_ctr_multi_raw(const uint64_t *table, size_t n_keys, const std::vector<CtrStreamIn> &streams, int rounds,
                           uint64_t *out, bool device_mem, int key_bits);
    std::vector<BitCt> aes_ctr_multi(const BitAt &table, size_t n_keys, const std::vector<CtrStreamIn> &streams,
                                     int rounds, int key_bits);
    void aes_cbc_multi_raw(const uint64_t *dtable, size_t n_keys, const std::vector<CbcStreamIn> &streams, int rounds,
                           uint64_t *out, bool device_mem, int key_bits);
    std::vector<BitCt> aes_cbc_multi(const BitAt &dtable, size_t n_keys, const std::vector<CbcStreamIn> &streams,
                                     int rounds, int key_bits);

    // ---- AES-CCM decryption of public frames over a key table (RFC 3610; aes_ccm.hpp; the reference
    // has no CCM).  The scope of the multi-key calls; a format refusal (nonce length, tag length, AAD >= 0xFF00, a
    // payload length that does not fit L bytes, data shorter than the tag) and rounds < 2 are TAE_E_PARAM before
    // any device work.  A single key is a table of one slot. ----
    struct CcmStreamIn {
        int32_t slot;
        const uint8_t *nonce;
        size_t nonce_len;
        const uint8_t *aad;
        size_t aad_len;
        const uint8_t *data;  // the ciphertext and the encrypted tag: len >= tag_len bytes
        size_t len;
    };
    struct CcmBits {
        std::vector<BitCt> plain, tag_diff;  // [sum (len - tag_len) * 8], [n_streams * 8 tag_len]
    };
    // the forward cipher over arbitrary public blocks [n_blocks][16] (host), block i under slot slots[i]:
    // out [n_blocks][128][bit_len], equal word for word to the cipher on trivial encryptions of the blocks
    void aes_pub_keystream_multi_raw(const uint64_t *table, size_t n_keys, const int32_t *slots, const uint8_t *blocks,
                                     size_t n_blocks, int rounds, uint64_t *out, bool device_mem, int key_bits);
    // out_plain [sum (len - tag_len)][8][bit_len], frames in order; out_tag_diff [n_streams][8 tag_len][bit_len] =
    // the recomputed tag xor the received one, all zero iff the frame is authentic
    void aes_ccm_multi_raw(const uint64_t *table, size_t n_keys, const std::vector<CcmStreamIn> &streams, int tag_len,
                           int rounds, uint64_t *out_plain, uint64_t *out_tag_diff, bool device_mem, int key_bits);
    // BitCt variant: the bits carry the levels and ids of aes_ccm_noise_schedule
    CcmBits aes_ccm_multi(const BitAt &table, size_t n_keys, const std::vector<CcmStreamIn> &streams, int tag_len,
                          int rounds, int key_bits);

    // ---- AES-GCM decryption of public frames under one key (SP 800-38D; aes_gcm.hpp; the reference
    // has no GCM).  1-bit WoP-PBS sets, gal-mul driver, 96-bit IVs, decryption (TAE_E_PARAM elsewhere).  Refusals
    // before any device work: an IV that is not 12 bytes, a tag_len outside 4, 8, 12 .. 16, rounds < 2, more hashed
    // blocks than n_powers (all TAE_E_PARAM); a row beyond the two-level chunk sum (TAE_E_NOISE).  A single key is a
    // table of one slot: these forms keep their argument checks and share the rest with the
    // key-table forms below, except that n_powers of the frame call is not bounded by 64 here. ----
    struct GcmFrameIn {
        const uint8_t *iv;
        size_t iv_len;
        const uint8_t *aad;
        size_t aad_len;
        const uint8_t *data;  // the ciphertext and the received tag: len >= tag_len bytes
        size_t len;
    };
    struct GcmBits {
        std::vector<BitCt> plain, tag_diff;  // [sum (len - tag_len) * 8], [n_frames * 8 tag_len]
    };
    // the power table H^1 .. H^n_powers [n_powers][128][bit_len] of the expanded key rk [W*32], n_powers in 1..=64
    void aes_ghash_key_raw(const uint64_t *rk, int n_powers, int rounds, uint64_t *out, bool device_mem, int key_bits);
    // BitCt variant: every table bit at noise^2 = 1 with a fresh id
    std::vector<BitCt> aes_ghash_key(const std::vector<const BitCt *> &expanded_key, int n_powers, int rounds, int key_bits);
    // out_plain [sum (len - tag_len)][8][bit_len], frames in order; out_tag_diff [n_frames][8 tag_len][bit_len] = the
    // recomputed tag xor the received one, all zero iff the frame is authentic
    void aes_gcm_raw(const uint64_t *rk, const uint64_t *hk, size_t n_powers, const std::vector<GcmFrameIn> &frames,
                     int tag_len, int rounds, uint64_t *out_plain, uint64_t *out_tag_diff, bool device_mem, int key_bits);
    // BitCt variant: the bits carry the levels and ids of aes_gcm_noise_schedule
    GcmBits aes_gcm(const std::vector<const BitCt *> &expanded_key, const std::vector<const BitCt *> &hk,
                    const std::vector<GcmFrameIn> &frames, int tag_len, int rounds, int key_bits);
    // ---- frames beyond one table: segmented GHASH (aes_gcm.hpp).  The scope and the refusals of the
    // calls above, and before any device work: seg outside 1 .. min(n_powers, 64), n_strides outside 1 .. 64, a frame of more
    // than n_strides + 1 segments (TAE_E_PARAM); an inner or a final row beyond 64 chunks (TAE_E_NOISE; never for
    // seg <= 31) ----
    // the stride key H^seg .. H^(n_strides seg) [n_strides][128][bit_len] of the table hk [n_powers][128][bit_len];
    // entry 0 is a copy of hk's block seg - 1
    void aes_ghash_stride_key_raw(const uint64_t *hk, size_t n_powers, size_t seg, int n_strides, uint64_t *out,
                                  bool device_mem);
    // BitCt variant: entry 0 clones the table's bits (their ids), every later bit is noise^2 = 1 with a fresh id
    std::vector<BitCt> aes_ghash_stride_key(const std::vector<const BitCt *> &hk, size_t seg, int n_strides);
    // the outputs of aes_gcm_raw for frames of up to (n_strides + 1) seg hashed blocks
    void aes_gcm_long_raw(const uint64_t *rk, const uint64_t *hk, size_t n_powers, const uint64_t *sk, size_t n_strides,
                          size_t seg, const std::vector<GcmFrameIn> &frames, int tag_len, int rounds, uint64_t *out_plain,
                          uint64_t *out_tag_diff, bool device_mem, int key_bits);
    // BitCt variant: the bits carry the levels and ids of aes_gcm_long_noise_schedule
    GcmBits aes_gcm_long(const std::vector<const BitCt *> &expanded_key, const std::vector<const BitCt *> &hk,
                         const std::vector<const BitCt *> &sk, size_t seg, const std::vector<GcmFrameIn> &frames,
                         int tag_len, int rounds, int key_bits);
    // ---- GCM over key tables: the calls above with a key table [n_keys][W*32][bit_len] and the power
    // tables [n_keys][n_powers][128][bit_len] of its slots.  The scope and the refusals of the single-key calls; a slot
    // outside 0..n_keys-1 is TAE_E_ARG, a slot no frame names is not read (neither table), and host memory uploads the
    // named slots alone.  Every output word, level and id is the single-key call's on that slot ----
    struct GcmStreamIn {
        int32_t slot;
        GcmFrameIn f;
    };
    void aes_ghash_key_multi_raw(const uint64_t *table, size_t n_keys, int n_powers, int rounds, uint64_t *out,
                                 bool device_mem, int key_bits);
    // BitCt variant: aes_ghash_key_noise_schedule per slot; table [n_keys * W*32]
    std::vector<BitCt> aes_ghash_key_multi(const std::vector<const BitCt *> &table, size_t n_keys, int n_powers, int rounds,
                                           int key_bits);
    void aes_gcm_multi_raw(const uint64_t *table, size_t n_keys, const uint64_t *htable, size_t n_powers,
                           const std::vector<GcmStreamIn> &frames, int tag_len, int rounds, uint64_t *out_plain,
                           uint64_t *out_tag_diff, bool device_mem, int key_bits);
    // BitCt variant: aes_gcm_noise_schedule per frame on its slot's key and table
    GcmBits aes_gcm_multi(const BitAt &table, size_t n_keys, const BitAt &htable, size_t n_powers,
                          const std::vector<GcmStreamIn> &frames, int tag_len, int rounds, int key_bits);
    // stage calls, no noise rule: squares / products of `count` field elements [count][128][bit_len]
    void gf128_square_raw(const uint64_t *in, size_t count, uint64_t *out, bool device_mem);
    void gf128_product_raw(const uint64_t *a, const uint64_t *b, size_t count, uint64_t *out, bool device_mem);

    // ---- AEAD open: the verdict bit and the verdict-gated payload (aead_open.hpp; the reference has
    // no AEAD).  Works on what the CCM and GCM calls return: plain [sum payload_lens][8][bit_len], frames in order, and
    // tag_diff [n_frames][8 tag_len][bit_len].  1-bit WoP-PBS sets only and a tag_len CCM or GCM accepts (TAE_E_PARAM
    // otherwise); n_frames == 0 is a no-op.  Refusals come before any device work and leave the stage times alone ----
    struct OpenBits {
        std::vector<BitCt> plain, ok;  // [sum payload_lens * 8] at level 9, [n_frames] at level 8, fresh ids
    };
    // ok [n_frames][bit_len]: 1 iff every difference bit of the frame is 0.  The raw forms replay the schedule for
    // inputs at the parameter set's cap
    void aead_verdict_raw(const uint64_t *tag_diff, size_t n_frames, int tag_len, uint64_t *ok, bool device_mem);
    // out_plain [sum payload_lens][8][bit_len] (not plain): the payload where ok = 1, zeros where ok = 0; payload_lens
    // is a host array
    void aead_open_raw(const uint64_t *plain, const size_t *payload_lens, const uint64_t *tag_diff, size_t n_frames,
                       int tag_len, uint64_t *out_plain, uint64_t *out_ok, bool device_mem);
    // BitCt variant: replays aead_open_noise_schedule on the inputs' levels (TAE_E_NOISE above the cap)
    OpenBits aead_open(const std::vector<const BitCt *> &plain, const size_t *payload_lens,
                       const std::vector<const BitCt *> &tag_diff, size_t n_frames, int tag_len);

    // ---- 8-bit model (src/tfhe/shortint_woppbs_8bit.rs, fhe_impls/shortint_woppbs_8bit.rs) ----
    size_t bit_len() const { return params().bit_len(); }
    // FheContext::bootstrap_from_bits over G bytes: bits [G][8][n+1] -> int ciphertexts [G][K+1]
    void bootstrap_from_bits_raw(const uint64_t *bits, size_t groups, const Lut &lut, uint64_t *out, bool device_mem);
    // FheContext::extract_bits_from_ciphertext over G ints: [G][K+1] -> [G][8][n+1]
    void extract_bits_raw(const uint64_t *ints, size_t groups, uint64_t *out, bool device_mem);

    // ---- shortint_1bit model (src/tfhe/shortint_1bit.rs; param set SHORTINT_1BIT), raw arrays ----
    // FheContext::bootstrap over B bits [B][n+1] with test vectors tvs [n_tv][(k+1)N] (bit b takes b % n_tv)
    void s1_bootstrap_raw(const uint64_t *in, size_t B, const uint64_t *tvs, size_t n_tv, uint64_t *out, bool device_mem);
    // FheContext::packing_keyswitch: count bits -> one GLWE [(k+1)N]
    void s1_packing_keyswitch_raw(const uint64_t *cts, size_t count, uint64_t *glwe, bool device_mem);
    // test_vector_from_ciphertexts over B pairs (ct0[b], ct1[b]) -> [B][(k+1)N]
    void s1_test_vectors_from_ciphertexts_raw(const uint64_t *ct0, const uint64_t *ct1, size_t B, uint64_t *tvs,
                                              bool device_mem);
    // calculate_multivariate_function for n_fn functions (f_tables [n_fn][2^nbits], host, 0/1 values) of
    // G groups of nbits bits [G][nbits][n+1] -> [G][n_fn][n+1]
    void s1_multivariate_raw(const uint64_t *bits, size_t G, int nbits, const uint64_t *f_tables, int n_fn,
                             uint64_t *out, bool device_mem);

    // ---- packed ciphertext I/O (glwe_pack.hpp): params_sqrd_lvl_64 only, TAE_E_PARAM elsewhere.
    // count bits <-> ceil(count / N) GLWEs [(k+1)N]; count == 0 is TAE_E_ARG ----
    // sample extraction of client-made GLWEs into big-key bits [count][K+1] (exact: no noise added)
    void unpack_bits_raw(const uint64_t *glwes, size_t count, uint64_t *bits, bool device_mem);
    // BitCt variant (host GLWEs): every bit at noise^2 = 1 with a fresh id, as a fresh encryption
    std::vector<BitCt> unpack_bits(const uint64_t *glwes, size_t count);
    // GLWE g = sum_j X^j PFKS_{q=k}(bit g N + j).  The result is terminal: for the client or for storage
    void pack_bits_raw(const uint64_t *bits, size_t count, uint64_t *glwes, bool device_mem);
    void pack_bits(const std::vector<const BitCt *> &bits, uint64_t *glwes);
    // the per-bit GLWEs before the sum [count][(k+1)N]
    void pack_pfks_raw(const uint64_t *bits, size_t count, uint64_t *glwes, bool device_mem);
    void require_pack(size_t count) const;

    // ---- the engine's stages one at a time (tae_stage_*): no noise rule.  Shapes as in engine.hpp; a LUT is in the
    // memory kind of the call; a host output is zero where the stage writes nothing ----
    void keyswitch_raw(const uint64_t *in, size_t count, uint64_t *out, bool device_mem);
    void pbs_shift_boolean_raw(const uint64_t *small, size_t count, int level, uint64_t *big, bool device_mem);
    void bootstrap_raw(const uint64_t *small, size_t count, const uint64_t *lut_glwe, uint64_t *big, bool device_mem);
    void pfks_ggsw_raw(const uint64_t *big, size_t count, int level, uint64_t *ggsw, bool device_mem);
    void ggsw_fourier_raw(const uint64_t *ggsw, size_t count, cplx *ggsw_f, bool device_mem);
    void vertical_packing_raw(const cplx *ggsw_f, size_t groups, int n_in, const uint64_t *lut, int n_out, uint64_t *out,
                              bool device_mem);
    // lhs += rhs over count ciphertexts [count][bit_len]: tae_xor_batch after its noise rule
    void xor_raw(uint64_t *lhs, const uint64_t *rhs, size_t count, bool device_mem);

  private:
    void require_s1() const;
    class Staged;  // the staging scope of an entry point (model.cpp)
    std::vector<BitCt> sbox_pbs_key_schedule(const std::vector<const BitCt *> &key);
    std::vector<NoiseLevel> block_noise_schedule(AesDriver driver, const std::vector<NoiseLevel> &rk,
                                                 const std::vector<NoiseLevel> &block, int rounds, int nr = 10) const;
    int require_key_bits(int key_bits, AesDriver driver) const;
    int require_key_expand(int key_bits) const;
    int check_ctr(uint64_t first_counter, size_t n_blocks, int rounds, int key_bits) const;
    int require_inverse(int rounds, int key_bits) const;
    int require_multi(int key_bits, int rounds) const;
    // the frames of a CCM / GCM call through the engine, host or device arrays
    void ccm_call(const uint64_t *table, std::vector<int32_t> slots, const std::vector<CcmFrame> &frames,
                  const std::vector<CcmStreamIn> &streams, int tag_len, int rounds, int nr, size_t key_cts,
                  uint64_t *out_plain, uint64_t *out_tag_diff, bool device_mem);
    // the frame list of the engine's GCM calls and the u64 words of both outputs; In is GcmFrameIn or GcmStreamIn.
    // gcm_staging leaves every slot 0 (one key); gcm_call writes the staged slot of every frame
    struct GcmStaging {
        std::vector<Engine::GcmFrameIn> ein;
        size_t plain_words = 0, tag_words = 0;
    };
    template <class In>
    GcmStaging gcm_staging(const std::vector<GcmFrame> &frames, const std::vector<In> &in, int tag_len) const;
    // A single key is a table of one slot (n_keys = 1, every slot 0) and, with key_table = false, keeps its own bound:
    // its power table may hold more than 64 powers
    void gcm_call(const uint64_t *table, size_t n_keys, bool key_table, const uint64_t *htable, size_t n_powers,
                  std::vector<int32_t> slots, GcmStaging g, int rounds, int nr, size_t key_cts, uint64_t *out_plain,
                  uint64_t *out_tag_diff, bool device_mem);
    // the power tables of n_keys slots after a form's own argument checks: raw arrays, and handles
    void ghash_key_raw_call(const uint64_t *table, size_t n_keys, int n_powers, int rounds, int nr, size_t key_cts,
                            uint64_t *out, bool device_mem);
    std::vector<BitCt> ghash_key_bits(const std::vector<const BitCt *> &table, size_t n_keys, int n_powers, int rounds,
                                      int nr, size_t key_cts);
    void gcm_long_call(const uint64_t *rk, const uint64_t *hk, size_t n_powers, const uint64_t *sk, size_t n_strides,
                       size_t seg, const std::vector<GcmFrame> &frames, const std::vector<GcmFrameIn> &in, int tag_len,
                       int rounds, int nr, size_t key_cts, uint64_t *out_plain, uint64_t *out_tag_diff, bool device_mem);
    // the AEAD open's three tables (or8, nor8, gate), built once per context and kept on the host
    struct OpenLuts {
        Lut or8, nor8, gate;
    };
    const OpenLuts &open_luts();
    std::once_flag open_once_;
    OpenLuts open_luts_;
    void open_call(const uint64_t *plain, const GatePlan *gate, const uint64_t *tag_diff, const VerdictPlan &verdict,
                   uint64_t *out_plain, uint64_t *out_ok, bool device_mem);
    void run_aes_ctr(const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter, size_t n_blocks, int rounds,
                     const uint8_t *data, size_t out_bytes, uint64_t *out, bool device_mem, int nr);
    void run_aes_blocks(AesDriver driver, const uint64_t *d_rk, const uint64_t *d_in, size_t n_blocks, int rounds,
                        uint64_t *d_out, int nr);
    std::unique_ptr<Engine> engine_;
    std::mutex mu_;
};

// Noise bookkeeping of the AES round function on metadata only: returns output noise levels
// (per bit) or throws ModelError exactly where the reference would panic.
// nr = 10 / 12 / 14 (here and in the replays below): rk has 4 (nr + 1) words and the last round key is word 4 nr.
std::vector<NoiseLevel> aes_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &block,
                                           int rounds, uint64_t max_noise_sq, int nr = 10);
// fhe_sbox_pbs over the 1-bit model: raises TAE_E_INDEP at the first MixColumns (rounds >= 2).
std::vector<NoiseLevel> sbox_pbs_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &block,
                                                int rounds, uint64_t max_noise_sq);
// The same for fhe_sbox_pbs with the 8-bit model (additive shortint NoiseLevel, max 11; SubBytes
// outputs are NOMINAL = 1).
std::vector<NoiseLevel> aes8_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &block,
                                            int rounds, uint64_t max_noise_level);

// The inverse cipher (aes_inv.hpp) on metadata, ONE block: dk [44*32], block [128] -> output levels [128].
// CBS outputs are noise^2 = 8 with fresh ids: a middle round is 4 * 8 + the key bit, the output 8 + the key bit.
std::vector<NoiseLevel> aes_decrypt_noise_schedule(const std::vector<NoiseLevel> &dk, const std::vector<NoiseLevel> &block,
                                                   int rounds, uint64_t max_noise_sq, int nr = 10);
// The decryption-key derivation on metadata: rk [44*32] -> dk [44*32]; the 4-term sums (noise^2 = 32) are
// validated, words 4..39 come out of the identity bootstrap at noise^2 = 1 with fresh ids.
std::vector<NoiseLevel> aes_decrypt_key_noise_schedule(const std::vector<NoiseLevel> &rk, uint64_t max_noise_sq,
                                                       int nr = 10);
// The key expansion (FIPS-197 5.2) on metadata: key [nk*32], nk = 4 / 6 / 8 -> rk [4 (nk + 7) * 32].  The word
// before its identity bootstrap is rk[i-nk] + 8 on SubWord steps and rk[i-nk] + rk[i-1] otherwise (validated);
// words below nk keep the key's levels and ids, every later word is noise^2 = 1 with fresh ids.
std::vector<NoiseLevel> aes_key_expand_noise_schedule(const std::vector<NoiseLevel> &key, int nk, uint64_t max_noise_sq);

// XTS (aes_xts.hpp) on metadata.  The tweak: the forward schedule of rk2 on a trivial block (output 8 + 1,
// validated), then the identity bootstrap: [128] at noise^2 = 1 with fresh ids.
std::vector<NoiseLevel> aes_xts_tweak_noise_schedule(const std::vector<NoiseLevel> &rk2, int rounds, uint64_t max_noise_sq,
                                                     int nr = 10);
// ONE block, index j of its unit: mask bit o = the sum of the tweak bits in row o of A_j (level = the row weight,
// at most w(j)); round 0 = mask + dk1's last round key; output = 8 + the key bit + the mask bit, carrying the ids
// of the tweak bits in its row.  dk1 [4 (nr + 1) * 32], tweak [128] -> [128]
std::vector<NoiseLevel> aes_xts_noise_schedule(const std::vector<NoiseLevel> &dk1, const std::vector<NoiseLevel> &tweak,
                                               uint64_t j, int rounds, uint64_t max_noise_sq, int nr = 10);

// CCM (aes_ccm.hpp) on metadata, ONE frame under the expanded key rk [4 (nr + 1) * 32].  Squared levels per bit:
// a circuit-bootstrap output is 8 with a fresh id; a plaintext bit is 8 + the last round key's bit; round 0 of a
// chain step is X' + the last round key's bit + rk_0's (8 + 1 + 1) at a public byte and X' + S' + rk_0's
// (8 + 8 + 1) at a payload byte, where the two last-round-key terms are removed, not added; a tag-difference bit
// is X'_last + S'_0 = 16 and holds no key bit.  rounds < 2 is TAE_E_PARAM.
struct CcmNoise {
    std::vector<NoiseLevel> plain, tag_diff;           // [payload_len * 8], [8 M]
    std::vector<std::vector<uint64_t>> step_round0;  // [n_mac - 1][128]: the squared levels of every step's round 0
};
CcmNoise aes_ccm_noise_schedule(const std::vector<NoiseLevel> &rk, const CcmFrame &frame, int rounds,
                                uint64_t max_noise_sq, int nr = 10);

// GCM (aes_gcm.hpp) on metadata.  The power table of rk [4 (nr + 1) * 32]: E_K(0) (8 + 1, validated) and its refresh;
// a square is the row sum of its operand's bits (at most 5) and a refresh; a product is 7168 partial bits at 8 with
// fresh ids, chunk sums of at most 7 (56), a refresh, the reduction (at most 34) and a refresh.  Every sum is
// validated; every table bit comes out at noise^2 = 1 with a fresh id.  The largest level of each kind is recorded.
struct GhashKeyNoise {
    std::vector<NoiseLevel> table;  // [n_powers * 128]
    uint64_t max_chunk = 0, max_reduced = 0, max_square = 0;
};
GhashKeyNoise aes_ghash_key_noise_schedule(const std::vector<NoiseLevel> &rk, int n_powers, int rounds,
                                           uint64_t max_noise_sq, int nr = 10);
// ONE frame under rk and the table hk [n_powers * 128]: a payload bit is 8 + the last round key's bit; a chunk is the
// E(J0) bit (8 + 1) plus at most 55 table bits, or at most 64 table bits; a tag-difference bit is the sum of its
// row's refreshed chunks: its level is their number, its ids are fresh, it holds no key bit.  m > n_powers and
// rounds < 2 are TAE_E_PARAM, a row of more than 64 chunks TAE_E_NOISE.
struct GcmNoise {
    std::vector<NoiseLevel> plain, tag_diff;  // [data_len * 8], [8 tag_len]
    uint64_t max_chunk = 0;
};
// The frames of a call over key tables, host only and before any device work: the format refusals of the single-key
// call (TAE_E_PARAM), a slot outside 0..n_keys-1 (TAE_E_ARG), more hashed blocks than n_powers (TAE_E_PARAM), a row
// beyond 64 chunks (TAE_E_NOISE).  Returns the frames and writes their slots
std::vector<GcmFrame> gcm_multi_frames(const std::vector<Context::GcmStreamIn> &in, size_t n_keys, size_t n_powers,
                                       int tag_len, std::vector<int32_t> &slots);
GcmNoise aes_gcm_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &hk, const GcmFrame &frame,
                                int rounds, uint64_t max_noise_sq, int nr = 10);
// Segmented GHASH.  The stride key of the table hk [n_powers * 128]: entry 0 keeps the levels and ids
// of hk's block seg - 1 and enters no sum with a table bit; the rest is the schedule above on that base, every bit at
// noise^2 = 1 with a fresh id.  seg outside 1 .. min(n_powers, 64) and n_strides outside 1 .. 64 are TAE_E_PARAM.
GhashKeyNoise aes_ghash_stride_key_noise_schedule(const std::vector<NoiseLevel> &hk, size_t seg, int n_strides,
                                                  uint64_t max_noise_sq);
// ONE frame under rk, hk and the stride key sk [n_strides * 128].  An inner chunk is at most 64 table bits; an inner
// row the sum of its refreshed chunks (at most 64), then 1 after its refresh; a product as the key schedule replays
// it; the first final chunk the E(J0) bit (8 + 1) plus at most 55 level-1 bits (table bits and product bits), later
// ones at most 64; a tag-difference bit its chunk count with fresh ids and no key bit; a payload bit 8 + 1.  Of sk
// only the length is read: a stride power enters nothing but a product, whose 256 operand bits each go through the
// circuit bootstrap, so its levels and ids reach no sum (the key schedules replay a product the same way).
struct GcmLongNoise {
    std::vector<NoiseLevel> plain, tag_diff;  // [data_len * 8], [8 tag_len]
    uint64_t max_inner_chunk = 0, max_inner_row = 0, max_part_chunk = 0, max_reduced = 0, max_chunk = 0;
};
GcmLongNoise aes_gcm_long_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &hk,
                                         const std::vector<NoiseLevel> &sk, size_t seg, const GcmFrame &frame, int rounds,
                                         uint64_t max_noise_sq, int nr = 10);

// The AEAD open (aead_open.hpp) on metadata: plain [n_bytes * 8] (empty: the verdict alone), diff [n_frames * 8 tag_len].
// A circuit bootstrap's outputs are at its input bit count with fresh ids (Lemma 3.2), whatever its inputs hold: a
// verdict-level output is at 8, the padding is trivial, a gated payload bit is at 9 and no output holds a key bit.  Every
// input of every bootstrap must be at or below the cap: TAE_E_NOISE otherwise.
struct AeadOpenNoise {
    std::vector<NoiseLevel> plain, ok;  // [n_bytes * 8], [n_frames]
};
AeadOpenNoise aead_open_noise_schedule(const std::vector<NoiseLevel> &plain, const std::vector<NoiseLevel> &diff,
                                       const VerdictPlan &verdict, const GatePlan &gate, uint64_t max_noise_sq);

// Counter mode on the 1-bit model: output noise [n_blocks][128] of the gal-mul schedule for trivial counter
// blocks.  rounds >= 2: aes_noise_schedule per block.  rounds == 1: the final SubBytes runs on the plan's
// groups, so outputs that read the same group carry the same component id.
std::vector<std::vector<NoiseLevel>> aes_ctr_noise_schedule(const std::vector<NoiseLevel> &rk, const CtrPlan &plan,
                                                            size_t n_blocks, int rounds, uint64_t max_noise_sq,
                                                            int nr = 10);

}  // namespace tae
