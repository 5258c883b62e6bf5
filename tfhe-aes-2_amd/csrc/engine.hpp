// Device engine: server keys resident in HBM and the batched hot-path stages as HIP kernels.
//
// Reference hot path: FheContext::circuit_bootstrap
// (src/tfhe/shortint_woppbs_1bit.rs:292-336) = per input bit extract_dual_bit_from_bit
// (:339-363 -> tfhe extract_bits = one LWE keyswitch), then tfhe
// circuit_bootstrap_boolean_vertical_packing (homomorphic_shift_boolean PBS, k+1 private
// functional keyswitches into a GGSW, forward FFT of the GGSW, vertical-packing blind rotation,
// sample extraction).  Every stage here is batched over all bits of all SBOXes of a round.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <deque>
#include <string>
#include <vector>

#include "client.hpp"
#include "cplx.hpp"
#include "aead_open.hpp"
#include "aes_ccm.hpp"
#include "aes_gcm.hpp"
#include "aes_xts.hpp"
#include "ctr_plan.hpp"
#include "devbuf.hpp"
#include "kslots.hpp"
#include "params.hpp"
#include "rowsum.hpp"

namespace tae {

// Timing of the most recent batched call, per stage (ms, HIP events on the engine stream).
struct StageTimes {
    float keyswitch = 0, pbs = 0, pfks = 0, ggsw_fft = 0, vertical_packing = 0, extract = 0, linear = 0;
    float pack = 0;  // the last pack_bits call (keyswitch slice + rotate-and-sum); the other slots keep their values
    int pbs_launches = 0;  // CBS-level PBS launches (one homomorphic_shift_boolean batch each)
    // the throughput blind-rotation kernel alone (br512x4 launches inside the PBS stage, without the
    // br512lat remainder) and the ciphertexts those launches processed
    float pbs_main = 0;
    double pbs_main_cts = 0;
    // clock mode (set_timing(2)): median effective shader clock over the workgroups of each throughput
    // blind-rotation launch (br512x4, or br1024 with two ciphertexts per workgroup), summed over launches
    double pbs_clock_ghz_sum = 0;
    int pbs_clock_launches = 0;
};
enum Stage { ST_KS = 0, ST_PBS, ST_PFKS, ST_FFT, ST_VP, ST_EXTRACT, ST_LINEAR, ST_PBS_MAIN, ST_PACK };

class Engine {
  public:
    // Uploads the standard-domain keys and converts the BSK to the Fourier domain on device.
    Engine(const ServerKeyRaw &keys, int device);
    // Attach to keys already resident on this device (e.g. broadcast over RCCL); the standard
    // BSK is converted in place into an engine-owned Fourier buffer.  Pointers must stay valid.
    Engine(const Params &p, int device, const uint64_t *d_ksk, const uint64_t *d_bsk,
           const uint64_t *d_pfpksk);
    ~Engine();
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;

    const Params &params() const { return p_; }
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }

    // ---- batched stages, all pointers device-resident ----
    // keyswitch_lwe_ciphertext: [B][K+1] -> [B][n+1]
    void keyswitch(const uint64_t *d_in, uint64_t *d_out, size_t B);
    // homomorphic_shift_boolean at cbs level `level`: [B][n+1] -> [B][K+1]
    void pbs_shift_boolean(const uint64_t *d_small, uint64_t *d_big, size_t B, int level);
    // generic FourierLweBootstrapKey::bootstrap with LUT GLWEs [(k+1)N]: ciphertext b takes
    // d_lut_glwe + (b % lut_mod) (k+1)N (lut_mod 1: one LUT for the batch; lut_mod > 1, a test vector per
    // ciphertext, runs on br512x4<7, true, 6> for shortint_1bit and on the generic pbs_kernel otherwise)
    void bootstrap(const uint64_t *d_small, const uint64_t *d_lut_glwe, uint64_t *d_big, size_t B,
                   uint64_t body_add, uint64_t out_add, size_t lut_mod = 1);
    // private functional keyswitches of level `level`: [B][K+1] -> GGSW rows of that level in
    // d_ggsw [B][cbs_l][k+1][(k+1)N]
    void pfks_into_ggsw(const uint64_t *d_big, uint64_t *d_ggsw, size_t B, int level);
    // ---- packed ciphertext I/O (glwe_pack.hpp), params_sqrd_lvl_64 only ----
    // sample extraction of `count` packed bits: GLWEs [ceil(count / N)][(k+1)N] -> big-key LWEs [count][K+1]
    void unpack_bits(const uint64_t *d_glwes, size_t count, uint64_t *d_bits);
    // the private functional keyswitch of key q = k alone (plaintext polynomial -1: coefficient 0 of the GLWE
    // carries the LWE's phase): [B][K+1] -> [B][(k+1)N], on the path pfks_into_ggsw takes for B ciphertexts
    void pack_pfks(const uint64_t *d_big, size_t B, uint64_t *d_out);
    // GLWE g = sum_j X^j pack_pfks(bit g N + j): [count][K+1] -> [ceil(count / N)][(k+1)N], in chunks of at most
    // glwe_pack::kChunkBits bits of keyswitch scratch
    void pack_bits(const uint64_t *d_bits, size_t count, uint64_t *d_glwes);
    // fill_with_forward_fourier: [B][cbs_l][k+1][(k+1)N] -> [B][cbs_l][k+1][k+1][M]
    void ggsw_to_fourier(const uint64_t *d_ggsw, cplx *d_ggsw_f, size_t B);
    // vertical_packing for each group of n_in GGSWs: d_ggsw_f [G][n_in][...], d_lut
    // [n_out][N], out [G][n_out][K+1]
    void vertical_packing(const cplx *d_ggsw_f, size_t G, int n_in, const uint64_t *d_lut, int n_out,
                          uint64_t *d_out);
    // LUTs with input_bits > log2 N: CMux tree over the first `tree` GGSWs, then the blind rotation
    void vertical_packing_tree(const cplx *d_ggsw_f, size_t G, int n_in, int tree, const uint64_t *d_lut, int n_out,
                               uint64_t *d_out);
    // FheContext::circuit_bootstrap over G groups: bits [G][n_in][K+1] -> [G][n_out][K+1]
    void circuit_bootstrap(const uint64_t *d_bits, size_t G, int n_in, const uint64_t *d_lut,
                           int n_out, uint64_t *d_out);
    // circuit_bootstrap_boolean_vertical_packing on small-key bits (no keyswitch):
    // [G][n_in][n+1] -> [G][n_out][K+1]  (8-bit model: WopbsKey::circuit_bootstrapping_vertical_packing)
    void cbs_vp(const uint64_t *d_small_bits, size_t G, int n_in, const uint64_t *d_lut, int n_out,
                uint64_t *d_out);
    // tfhe wop_pbs::extract_bits: big-key [B][K+1] -> small-key bits [B][nbits][n+1], MSB first
    // (8-bit model extract_bits_from_ciphertext, shortint_woppbs_8bit.rs:268-296)
    void extract_bits(const uint64_t *d_in, size_t B, int delta_log, int nbits, uint64_t *d_out);
    // Byte::bootstrap_with_lut (fhe_impls/shortint_woppbs_8bit.rs:37-42) over G bytes:
    // [G][8][n+1] -> [G][8][n+1] through one 8-bit int ciphertext per byte
    void bootstrap_bytes8(const uint64_t *d_bytes, size_t G, const uint64_t *d_lut, uint64_t *d_out);
    // fhe_sbox_pbs::encrypt_block_for_rounds over nb blocks of small-key bits (8-bit model):
    // rk [44*32][n+1], blocks [nb][128][n+1]
    void aes8_encrypt_blocks(const uint64_t *d_rk, const uint64_t *d_blocks, size_t nb, int rounds,
                             uint64_t *d_out);

    // ---- AES driver (fhe_sbox_gal_mul_pbs::encrypt_block_for_rounds over many blocks) ----
    // rk [44*32][K+1] (expanded key words, word-major, MSB-first bits), blocks [nb][128][K+1].
    // nr = 10 / 12 / 14 is the round count of the key size (AES-128 / 192 / 256), here and in the modes below:
    // rk has 4 (nr + 1) words, rounds may go up to nr, and a run of `rounds` rounds uses round keys 0,
    // 1..rounds-1 and nr (the last one at word 4 nr)
    // d_key_of != nullptr (device, [nb]) is the keyed form: d_rk is a key table and block i reads the round keys
    // of slot d_key_of[i] at d_rk + d_key_of[i] * key_stride (the same for aes_decrypt_blocks)
    void aes_encrypt_blocks(const uint64_t *d_rk, const uint64_t *d_blocks, size_t nb, int rounds,
                            uint64_t *d_out, int nr = 10, const int32_t *d_key_of = nullptr, size_t key_stride = 0);
    // key expansion on the device (FIPS-197 5.2, figure 11; fhe_sbox_gal_mul_pbs::key_schedule for nk = 4):
    // key [nk*32][K+1], nk = 4 / 6 / 8 -> rk [4 (nk + 7) * 32][K+1].  Words below nk are copied; word i is
    // rk[i-nk] + rk[i-1], with SubWord (one 4-group 8 -> 8 bootstrap), RotWord and Rcon when i % nk == 0 and
    // SubWord alone when nk == 8 and i % 8 == 4, then one identity bootstrap of its 32 bits.  1-bit model only
    void aes_key_expand(const uint64_t *d_key, int nk, uint64_t *d_rk);

    // ---- AES-128-CTR with public counters (main.rs:108-128; ctr_plan.hpp) ----
    // The keystream blocks of one plan (nb blocks) for the 1-bit model: round 0 builds the plan's U
    // deduplicated SubBytes inputs from rk0, round 1 bootstraps those U groups only and the linear layer
    // reads them through the plan's map; rounds 2.. run as in aes_encrypt_blocks.  No input ciphertexts.
    // Writes the first out_bytes (<= 16 nb) keystream bytes [out_bytes][8][K+1]; with d_data (out_bytes
    // public bytes on the device) each output is keystream xor data (transciphering).
    void aes_ctr_blocks(const uint64_t *d_rk, const CtrPlan &plan, size_t nb, int rounds, const uint8_t *d_data,
                        size_t out_bytes, uint64_t *d_out, int nr = 10);
    // the same for the 8-bit model (small-key bits [n+1], bootstrap_bytes8 + the gf_256_mul network)
    void aes8_ctr_blocks(const uint64_t *d_rk, const CtrPlan &plan, size_t nb, int rounds, const uint8_t *d_data,
                         size_t out_bytes, uint64_t *d_out, int nr = 10);
    // counters first_counter .. first_counter + nb - 1 in consecutive chunks of ctr_chunk_ blocks, each with
    // its own plan, on the model of the parameter set (1-bit or 8-bit)
    void aes_ctr(const uint64_t *d_rk, const uint8_t iv[8], uint64_t first_counter, size_t nb, int rounds,
                 const uint8_t *d_data, size_t out_bytes, uint64_t *d_out, int nr = 10);

    // ---- AES-128 inverse cipher on the 1-bit model (FIPS-197 5.3; the reference has no decryption).  The
    // algorithm is in aes_inv.hpp: InvSubBytes and InvMixColumns' multiples {14,11,13,9} in one 8 -> 32 circuit
    // bootstrap per byte and middle round, one 8 -> 8 for the last: `rounds` bootstraps per block, as encryption ----
    // dk [44*32][K+1] (aes_decrypt_key), blocks / out [nb][128][K+1]; inverts aes_encrypt_blocks(rounds): round
    // keys nr, rounds-1 .. 1, 0 of a key of 4 (nr + 1) words
    void aes_decrypt_blocks(const uint64_t *d_dk, const uint64_t *d_blocks, size_t nb, int rounds, uint64_t *d_out,
                            int nr = 10, const int32_t *d_key_of = nullptr, size_t key_stride = 0);
    // decryption key: words 0..3 and 40..43 copied, words 4r..4r+3 = InvMixColumns(rk[r]) by one 8 -> 32 bootstrap
    // of the 144 bytes (multiples only), the 4-term sums and one identity bootstrap of the 1152 bits.  d_dk != d_rk.
    // With nr: words 4 nr .. 4 nr + 3 are the last copy, and the middle is 16 (nr - 1) bytes, 128 (nr - 1) bits
    void aes_decrypt_key(const uint64_t *d_rk, uint64_t *d_dk, int nr = 10);
    // CBC with a public ciphertext: d_iv_data = iv[16] || nb blocks of ciphertext bytes on the device; out
    // [nb][128][K+1] = Dec(C_i) ^ C_{i-1}.  Round 0 and the last XOR come from the public bytes: no input ciphertexts
    void aes_cbc_transcipher(const uint64_t *d_dk, const uint8_t *d_iv_data, size_t nb, int rounds, uint64_t *d_out,
                             int nr = 10);

    // ---- XTS-AES decryption of a public ciphertext on the 1-bit model (aes_xts.hpp; the reference
    // has no XTS).  `rounds` applies to both ciphers ----
    // T = Enc_K2(tweak), refreshed by one identity bootstrap: rk2 [4 (nr + 1) * 32][K+1], d_tweaks [n][16] public
    // bytes on the device -> [n][128][K+1] at noise^2 = 1
    void aes_xts_tweaks(const uint64_t *d_rk2, const uint8_t *d_tweaks, size_t n, int rounds, uint64_t *d_out,
                        int nr = 10);
    // masks [nb][128][K+1] = alpha^j T of the blocks of an xts_plan (HOST, validated against n_units before the
    // launch) from tweak ciphertexts [n_units][128][K+1]: one row-sum launch
    void aes_xts_masks(const uint64_t *d_tweak_cts, size_t n_units, const RowPlan &plan, uint64_t *d_masks);
    // out [nb][128][K+1] = Dec_K1(C_b + M_b) + M_b: the tweak pass over the n_tweaks distinct tweaks (device bytes),
    // then per chunk of ctr_chunk_ blocks the masks, aes_decrypt_rounds on masks + public C and the last add.
    // Block b is block block_index[b] of the unit with tweak tweak_of[b] (HOST arrays, the caller checks the
    // range); d_data [nb][16] on the device
    void aes_xts_transcipher(const uint64_t *d_dk1, const uint64_t *d_rk2, const uint8_t *d_tweaks, size_t n_tweaks,
                             const int32_t *tweak_of, const uint64_t *block_index, const uint8_t *d_data, size_t nb,
                             int rounds, uint64_t *d_out, int nr = 10);

    // ---- AES-CCM decryption of public frames on the 1-bit model (aes_ccm.hpp; the reference has no
    // CCM).  `rounds` (>= 2) applies to every cipher call ----
    // One frame under slot `slot` of a key table: `data` = the frame's payload_len ciphertext bytes, `tag` its M
    // encrypted-tag bytes (HOST arrays, read during the call)
    struct CcmStreamIn {
        int32_t slot;
        const CcmFrame *frame;
        const uint8_t *data, *tag;
    };
    // The forward cipher over public blocks (HOST), block i under slot blocks[i].slot, in chunks of ctr_chunk_
    // blocks (pub_pass); writes each block's len bytes at out_byte of d_out
    void aes_pub_blocks_multi(const uint64_t *d_table, const std::vector<PubBlock> &blocks, int rounds, uint64_t *d_out,
                              int nr);
    // Pass 1: every stream's A_0, A_1 .. and B_0 as one batch of public blocks; the payload bits S_i + C go to
    // d_out_plain [sum payload_len][8][K+1], frames in order.  Then the CBC-MAC chain, one forward cipher per step
    // over the streams that still have a MAC block (the streams are ordered by decreasing block count inside the
    // call, so they are a prefix), its round 0 from aes_ccm_absorb_kernel.  d_out_tagdiff [n_streams][8 M][K+1] =
    // X_last + S_0 + U, frames in the caller's order; one M for the call
    void aes_ccm_transcipher(const uint64_t *d_table, const std::vector<CcmStreamIn> &streams, int rounds, int nr,
                             uint64_t *d_out_plain, uint64_t *d_out_tagdiff);

    // ---- AES-GCM decryption of public frames on the 1-bit model (aes_gcm.hpp; the reference has no
    // GCM).  A single key is a key table of one slot ----
    // squares of `count` field elements [count][128][K+1]: row sums, then one identity bootstrap (noise^2 = 1)
    void gf128_square(const uint64_t *d_in, size_t count, uint64_t *d_out);
    // products a_c b_c of `count` pairs, a / b / out [count][128][K+1]: the 256 operand bits of a pair are keyswitched
    // once and gathered as small ciphertexts into the 1024 groups of one 8 -> 7 cbs_vp call over all pairs; chunk
    // sums, identity bootstrap, reduction, identity bootstrap
    void gf128_product(const uint64_t *d_a, const uint64_t *d_b, size_t count, uint64_t *d_out);
    // One frame under slot `slot` of the key table and of the power tables (0 where the call has one key): `data` its
    // data_len ciphertext bytes, `tag` its tag_len received-tag bytes (HOST, read during the call)
    struct GcmFrameIn {
        int32_t slot;
        const GcmFrame *frame;
        const uint8_t *data, *tag;
    };
    // aes_gcm_transcipher_multi on a table of one slot: d_rk the expanded key, d_hk [n_powers][128][K+1] its power
    // table (ghash_key_multi of one slot), read in place.  A single key's n_powers is not bounded by 64
    void aes_gcm_transcipher(const uint64_t *d_rk, const uint64_t *d_hk, size_t n_powers,
                             const std::vector<GcmFrameIn> &frames, int rounds, int nr, uint64_t *d_out_plain,
                             uint64_t *d_out_tagdiff);
    // ---- frames beyond one table: segmented GHASH (aes_gcm.hpp) ----
    // the stride key H^seg, H^(2 seg) .. H^(n_strides seg) [n_strides][128][K+1] of the table d_hk: entry 0 a copy of
    // d_hk's block seg - 1, the rest the generations of gcm_power_schedule(n_strides) on that base
    void ghash_stride_key(const uint64_t *d_hk, size_t n_powers, size_t seg, int n_strides, uint64_t *d_out);
    // aes_gcm_transcipher's public pass, then the inner segments of all frames in batches of gcm_seg_batch_ (chunk
    // sums over the table's first seg powers, identity bootstrap, row sums, identity bootstrap, one product with the
    // segment's stride power from d_sk), then the final chunk sums over the table, E(J0) and the products, one
    // identity bootstrap and the differences.  The table's first min(seg, m) blocks are read where d_hk keeps them.
    // One key: every frame's slot is 0.  A frame of at most seg hashed blocks runs aes_gcm_transcipher's launches
    void aes_gcm_long_transcipher(const uint64_t *d_rk, const uint64_t *d_hk, size_t n_powers, const uint64_t *d_sk,
                                  size_t n_strides, size_t seg, const std::vector<GcmFrameIn> &frames, int rounds, int nr,
                                  uint64_t *d_out_plain, uint64_t *d_out_tagdiff);

    // ---- GCM over key tables: d_table [n_keys][4 (nr + 1) * 32][K+1] as in the multi-key batches
    // below, power tables [n_keys][n_powers][128][K+1].  Every output word equals the single-key call's on that slot ----
    // the power tables of all slots: E_K(0) of every slot in one public-block batch, one identity bootstrap over
    // n_keys * 128 bits, then every generation of gcm_power_schedule once: its squares of all keys in one
    // gcm_square_pass, its products of all keys in gcm_product_pass calls of at most gcm_seg_batch_ products
    // One table runs a generation's products in one pass: the power table of a single key is this call with n_keys = 1
    void ghash_key_multi(const uint64_t *d_table, size_t n_keys, int n_powers, int rounds, int nr, uint64_t *d_out);
    // One public-block batch over all frames' J0 and counter blocks, every block under its frame's slot: the payload
    // bits E(ctr) + C go to d_out_plain [sum data_len][8][K+1], frames in order, and E(J0) is kept by the second
    // placement.  Then one two-source row-sum launch for all chunks (A = d_htable in place, B = the kept E(J0) blocks;
    // the row base selects the slot's table), one identity bootstrap of the chunk bits and one row-sum launch for the
    // tag differences d_out_tagdiff [n_frames][8 tag_len][K+1].  Refused before any device work, the stage times
    // untouched: a slot outside 0 .. n_keys - 1, m > n_powers, a row of more than 64 chunks, rounds < 2, mixed tag
    // lengths, n_powers > 64.  A slot that no frame names is not read, neither its expanded key nor its power table
    void aes_gcm_transcipher_multi(const uint64_t *d_table, size_t n_keys, const uint64_t *d_htable, size_t n_powers,
                                   const std::vector<GcmFrameIn> &frames, int rounds, int nr, uint64_t *d_out_plain,
                                   uint64_t *d_out_tagdiff);

    // ---- AEAD open on the 1-bit model (aead_open.hpp; the reference has no AEAD).  The lookup tables
    // and the index tables are the call's: device arrays of its staging scope ----
    // d_tag_diff [n_frames][tag_bits][K+1] -> d_ok [n_frames][K+1], 1 iff every difference bit of the frame is 0: one
    // keyswitch of all difference bits, then per level of the plan (d_idx[l] its index table) a gather of small
    // ciphertexts and one 8 -> 1 cbs_vp over all frames, "OR of 8" below the last level and "NOR of 8" at it; a level's
    // outputs are keyswitched for the next
    void aead_verdict(const uint64_t *d_tag_diff, const VerdictPlan &plan, const std::vector<const int32_t *> &d_idx,
                      const uint64_t *d_lut_or8, const uint64_t *d_lut_nor8, uint64_t *d_ok);
    // d_plain [n_bytes][8][K+1], d_ok [n_frames][K+1] -> d_out [n_bytes][8][K+1] (not d_plain), byte g and-ed with the
    // verdict of its frame: the verdicts are keyswitched once, then passes of at most aead_gate_pass() bytes, each a
    // keyswitch, a gather (d_idx[pass]: aead_gate_pass_index) and one 9 -> 8 cbs_vp
    void aead_gate(const uint64_t *d_plain, const GatePlan &plan, const std::vector<const int32_t *> &d_idx,
                   const uint64_t *d_ok, const uint64_t *d_lut_gate, uint64_t *d_out);
    size_t aead_gate_pass() const { return (size_t)kOpenGateBlockBytes * ctr_chunk_; }

    // ---- multi-key batches on the 1-bit model (the reference has one key).  A key table is
    // [n_keys][4 (nr + 1) * 32][K+1], slot s an expanded (or decryption) key in the layout above.  The bootstraps
    // are per ciphertext, so bits of different keys share their launches; the linear layer reads the round key of
    // each block's slot.  key_of (HOST, [nb], every entry a valid slot: the caller checks) is uploaded
    // asynchronously.  A slot that no block refers to is not read.  Every output word equals the single-key path's. ----
    // keys [n_keys][nk*32][K+1] -> table; word i of all keys per step, so the chain of circuit bootstraps is as
    // long as for one key (50 / 54 / 65) whatever n_keys is
    void aes_key_expand_multi(const uint64_t *d_keys, int nk, size_t n_keys, uint64_t *d_table);
    // aes_decrypt_key for every slot in one pass of its three stages; d_dtable != d_table
    void aes_decrypt_key_multi(const uint64_t *d_table, size_t n_keys, uint64_t *d_dtable, int nr);
    void aes_encrypt_blocks_multi(const uint64_t *d_table, const int32_t *key_of, const uint64_t *d_blocks, size_t nb,
                                  int rounds, uint64_t *d_out, int nr);
    void aes_decrypt_blocks_multi(const uint64_t *d_dtable, const int32_t *key_of, const uint64_t *d_blocks, size_t nb,
                                  int rounds, uint64_t *d_out, int nr);
    // counter mode over the flattened blocks of several streams (ctr_flatten), in chunks of ctr_chunk_ blocks with
    // a CtrPlanMulti each; writes each block's len bytes at out_byte of d_out [sum len][8][K+1]; d_data (nullptr:
    // the keystream) holds the public bytes in output order
    void aes_ctr_multi(const uint64_t *d_table, const std::vector<CtrBlock> &blocks, int rounds, const uint8_t *d_data,
                       uint64_t *d_out, int nr);
    // CBC: d_cur / d_prev [nb][16] public bytes on the device, block i = Dec_{key_of[i]}(cur_i) ^ prev_i
    void aes_cbc_transcipher_multi(const uint64_t *d_dtable, const int32_t *key_of, const uint8_t *d_cur,
                                   const uint8_t *d_prev, size_t nb, int rounds, uint64_t *d_out, int nr);

    // ---- shortint_1bit model (src/tfhe/shortint_1bit.rs; param set SHORTINT_1BIT) ----
    // FheContext::bootstrap / bootstrap_assign (:257-291): PBS with test vector d_tvs + (b % lut_mod) (k+1)N, then the keyswitch
    // back to the small key: [B][n+1] -> [B][n+1]
    void s1_bootstrap(const uint64_t *d_in, const uint64_t *d_tvs, size_t lut_mod, uint64_t *d_out, size_t B);
    // keyswitch_lwe_ciphertext_into_glwe_ciphertext with the packing key, per ciphertext: [B][n+1] -> [B][(k+1)N]
    void s1_pks(const uint64_t *d_in, size_t B, uint64_t *d_out);
    // test_vector_from_ciphertexts (:392-492) over P pairs of packing keyswitches [2P][(k+1)N] -> [P][(k+1)N]
    void s1_tv_from_pks(const uint64_t *d_pks, size_t P, uint64_t *d_tv);
    // FheContext::packing_keyswitch (:240-254): count ciphertexts into one GLWE, #j at X^j
    void s1_pack(const uint64_t *d_in, int count, uint64_t *d_out);
    // calculate_multivariate_function (:538-547) / apply_selectors_rec (:549-576) for n_fn functions of the same nbits bits, over G groups:
    // bits [G][nbits][n+1] (MSB first), d_tvs [n_fn][2^(nbits-1)][(k+1)N] (generate_multivariate_test_vector)
    // -> [G][n_fn][n+1]; one batched bootstrap + packing step per selector level
    void s1_multivariate(const uint64_t *d_bits, size_t G, int nbits, const uint64_t *d_tvs, int n_fn, uint64_t *d_out);
    void s1_multivariate_chunk(const uint64_t *d_bits, size_t G, int nbits, const uint64_t *d_tvs, int n_fn,
                               uint64_t *d_out);
    // Shortint1BitSboxPbsAesEncrypt::encrypt_block_for_rounds over nb blocks: rk [44*32][n+1], blocks [nb][128][n+1]
    void s1_aes_encrypt_blocks(const uint64_t *d_rk, const uint64_t *d_blocks, size_t nb, int rounds, uint64_t *d_out);
    const uint64_t *s1_sbox_tvs() const { return d_s1_sbox_tv_; }  // [8][128][(k+1)N]
    const uint64_t *s1_identity_tv() const { return d_s1_id_tv_; }  // [(k+1)N]

    // ---- element-wise helpers ----
    void lwe_add(uint64_t *d_a, const uint64_t *d_b, size_t count);  // a += b (count u64)

    void synchronize();
    // Device-resident caller buffers (TAE_MEM_DEVICE) may have been written on any stream of the
    // caller (torch's current stream, an RCCL stream): wait for all device work before the engine's
    // non-blocking stream reads them.
    void order_after_caller();
    // TAE_MEM_DEVICE ordering: nullptr (default) = device-wide synchronize; otherwise the engine stream
    // waits on an event recorded on this caller stream (no host sync, other streams not waited for)
    void set_caller_stream(hipStream_t s) { caller_stream_ = s; }
    const StageTimes &last_times() const { return times_; }
    // The AES and mode drivers restart the stage times themselves.  A public call that reaches a stage directly (the
    // circuit bootstrap, the 8-bit and shortint_1bit entry points, unpack, the stage calls) brackets it with these: the
    // times and launch counts are that call's alone, and the spans it recorded are summed and their events returned
    // to the pool before the next call.  pack_bits does neither: its callers read the last batched call's slots
    void begin_call() { times_ = StageTimes{}; }
    void end_call() { collect_times(); }
    // the kernel of the last pfks_into_ggsw launch: "g6", "s16", "w32" or "w16" (K-layout GEMMs, TAE_PFKS_GEMM),
    // "rows" (6-bit row-tile GEMM), "u64" (scalar kernel), "none" before the first
    const char *last_pfks_kernel() const { return last_pfks_kernel_; }
    // 0 off, 1 HIP-event stage times, 2 stage times + in-kernel clock stamps of the blind rotations
    // (a diagnostic mode: each stamped launch is read back synchronously)
    void set_timing(int mode) {
        timing_ = mode != 0;
        clock_ = mode == 2;
    }

    // scratch sizing: reserve buffers for a circuit_bootstrap of `bits` input bits
    void reserve(size_t bits, size_t outputs);

    const uint64_t *lut_galmul() const { return d_lut24_; }  // 8 -> 24 (S, 2S', 3S')
    const uint64_t *lut_sbox() const { return d_lut8_; }     // 8 -> 8 SBOX
    // 8-bit model LUTs without padding (SBOX, identity), [N]
    const uint64_t *lut8_sbox() const { return d_wlut_sbox_; }
    const uint64_t *lut8_identity() const { return d_wlut_id_; }

  private:
    void init_common();
    void bsk_to_fourier(const uint64_t *d_bsk_std);

    Params p_;
    int device_;
    hipStream_t stream_ = nullptr;
    hipStream_t caller_stream_ = nullptr;
    hipEvent_t caller_ev_ = nullptr;
    std::vector<hipEvent_t> ev_pool_;
    // Destroys the events, then the stream.  Declared before every buffer: members go in reverse order, so the
    // buffers are freed first, after ~Engine or when a constructor throws
    struct Teardown {
        Engine &e;
        ~Teardown();
    } teardown_{*this};
    DevBuf<uint64_t> d_ksk_, d_pfpksk_;  // borrowed by the device-key constructor
    DevBuf<cplx> d_bsk_f_;
    DevBuf<cplx> d_twist_, d_untwist_, d_w_;
    DevBuf<uint64_t> d_lut_shift_;  // per cbs level: trivial GLWE with body = -alpha
    DevBuf<uint64_t> d_lut24_, d_lut8_;
    // inverse cipher (1-bit model): InvSbox * {14,11,13,9}, InvSbox, the multiples alone, the 1 -> 1 identity
    DevBuf<uint64_t> d_lut_inv32_, d_lut_inv8_, d_lut_mul32_, d_lut_id1_;
    void require_inverse(int rounds, int nr) const;
    void aes_decrypt_rounds(const uint64_t *d_dk, const uint64_t *d_blocks, const uint8_t *d_cur, size_t nb, int rounds,
                            const uint8_t *d_xor, uint64_t *d_out, int nr, const int32_t *d_key_of, size_t key_stride,
                            bool keep_times = false);
    // the forward cipher's one round loop (aes_engine.hip): every forward entry point fills an AesRun
    struct AesRun;
    void aes_forward(const AesRun &run);
    DevBuf<uint64_t> d_wlut_sbox_, d_wlut_id_;  // 8-bit model
    DevBuf<uint64_t> d_lut_x_;                  // extract_bits accumulators [nbits][glwe]
    int lut_x_delta_ = -1, lut_x_bits_ = 0;
    DevBuf<uint64_t> d_xbuf_, d_xsh_, d_xks_, d_xpbs_, d_ints_;
    int8_t mix_idx_[32][8] = {};
    // counter mode: blocks per device pass (TAE_CTR_CHUNK_BLOCKS; 1024 = the largest batch the tests pin),
    // the plan of the chunk in flight on the device, and the host plans the pending uploads read
    size_t ctr_chunk_ = 1024;
    DevBuf<uint16_t> d_ctr_groups_;
    DevBuf<int32_t> d_ctr_map_;
    std::vector<CtrPlan> ctr_plans_;
    void aes_ctr_chunk(const uint64_t *d_rk, const CtrPlan &plan, size_t nb, int rounds, const uint8_t *d_data,
                       size_t out_bytes, uint64_t *d_out, int nr);
    // multi-key batches: the per-block slots on the device and the host copy its pending upload reads; the
    // parallel arrays of a CtrPlanMulti and the plans of the chunks in flight
    DevBuf<int32_t> d_key_of_, d_ctr_gslot_, d_ctr_blen_;
    DevBuf<int64_t> d_ctr_bout_;
    std::vector<int32_t> key_of_host_;
    std::vector<CtrPlanMulti> ctr_mplans_;
    const int32_t *upload_key_of(const int32_t *key_of, size_t nb);
    // keep_out / keep_len / d_keep (CCM, GCM): a second placement of the same cipher outputs, into d_keep
    void aes_ctr_blocks_multi(const uint64_t *d_table, const CtrPlanMulti &plan, int rounds, const uint8_t *d_data,
                              uint64_t *d_out, int nr, const std::vector<int64_t> *keep_out = nullptr,
                              const std::vector<int32_t> *keep_len = nullptr, uint64_t *d_keep = nullptr);
    // The chunked public-block pass: a pub_plan and one aes_ctr_blocks_multi per chunk of ctr_chunk_ blocks, with
    // the chunk's part of the second placement if there is one.  The plans and the placement's per-chunk lists
    // live until the next pass; its arrays on the device
    void pub_pass(const uint64_t *d_table, const std::vector<PubBlock> &blocks, int rounds, const uint8_t *d_data,
                  uint64_t *d_out, int nr, const std::vector<int64_t> *keep_out = nullptr,
                  const std::vector<int32_t> *keep_len = nullptr, uint64_t *d_keep = nullptr);
    DevBuf<int64_t> d_pub_kout_;
    DevBuf<int32_t> d_pub_klen_;
    std::vector<std::vector<int64_t>> pub_kout_;
    std::vector<std::vector<int32_t>> pub_klen_;
    // Row sums (rowsum.hpp) over the sources A [n_a][K+1] and B [n_b][K+1]: validates the plan against n_a + n_b,
    // keeps it alive until the next call (the uploads are asynchronous) and launches once under ST_LINEAR: -> d_out
    // [n_rows][K+1].  n_b = 0 is rowsum_kernel over A, anything else rowsum2_kernel.  The plan's arrays on the device
    // and the host plans their pending uploads read
    void rowsum_pass(const uint64_t *d_a, size_t n_a, const uint64_t *d_b, size_t n_b, RowPlan plan, uint64_t *d_out);
    void rowsum_pass(const uint64_t *d_sources, size_t n_src, RowPlan plan, uint64_t *d_out) {
        rowsum_pass(d_sources, n_src, nullptr, 0, std::move(plan), d_out);
    }
    DevBuf<int32_t> d_rs_start_, d_rs_src_, d_rs_list_, d_rs_base_;
    DevBuf<uint8_t> d_rs_pub_;
    std::deque<RowPlan> rowsum_plans_;
    // CCM: S_0 and the chain value Xk of every stream [2 n][128][K+1], the arrays of the call on the device and
    // the host copies their pending uploads read
    DevBuf<uint64_t> d_ccm_keep_;
    DevBuf<uint8_t> d_ccm_bytes_;
    DevBuf<int64_t> d_ccm_src_;
    DevBuf<int32_t> d_ccm_slot_, d_ccm_order_;
    std::vector<uint8_t> ccm_bytes_;
    std::vector<int64_t> ccm_src_;
    std::vector<int32_t> ccm_slot_, ccm_order_;
    // GCM: the 8 -> 7 nibble-product table; what a call's chunk sums read next to the caller's power table (E(J0) of
    // every frame, then the segmented call's products and operand batch); two scratch arrays the row sums and the
    // refreshes alternate between; the operand bits and the partial bits of a product batch; the public bytes of a call
    // and the host copy their pending upload reads
    DevBuf<uint64_t> d_lut_gcm_;
    DevBuf<uint64_t> d_gcm_src_, d_gcm_a_, d_gcm_b_, d_gcm_ops_, d_gcm_ks_, d_gcm_parts_;
    DevBuf<uint8_t> d_gcm_bytes_;
    std::vector<uint8_t> gcm_bytes_;
    // products per gcm_product_pass (TAE_GCM_SEG_BATCH, 1 .. 64; 16 products are the largest cbs_vp launch the tests
    // pin).  It bounds the product scratch of both the segmented GHASH (inner segments per batch) and ghash_key_multi
    // (a generation's products of all keys), at about 0.21 GB a product
    size_t gcm_seg_batch_ = 16;
    void require_gcm() const;
    // the generations of gcm_power_schedule(n) on the tables [n][128][K+1] that start at the blocks `tabs` of d_base
    // [n_blocks][128][K+1], entry 0 of each the base: one square pass and the product passes per generation for all
    // tables.  Several tables split a generation's products at gcm_seg_batch_; one table runs them in one pass
    void gcm_power_generations(uint64_t *d_base, size_t n_blocks, const std::vector<size_t> &tabs, int n);
    // the layout checks and payload offsets of a call's frames; returns the payload bytes
    size_t gcm_frame_offsets(const std::vector<GcmFrameIn> &frames, std::vector<int64_t> &off) const;
    // the public blocks of a call: the ciphertext bytes up, the counters into d_out_plain, E(J0) of frame s into block
    // s of d_j0; the blocks of a frame run under its slot of the key table
    void gcm_public_pass(const uint64_t *d_table, const std::vector<GcmFrameIn> &frames, const std::vector<int64_t> &off,
                         size_t total, int rounds, int nr, uint64_t *d_out_plain, uint64_t *d_j0);
    // the short-frame call behind both of its doors: the plans (every index within int32_t), the public pass, the tail
    void gcm_frames_pass(const uint64_t *d_table, size_t n_keys, const uint64_t *d_htable, size_t n_powers,
                         const std::vector<GcmFrameIn> &frames, int rounds, int nr, uint64_t *d_out_plain,
                         uint64_t *d_out_tagdiff);
    // GHASH + E(J0) + the received tag: the plan's chunk sums over A and B, one identity bootstrap, the differences.
    // d_gcm_a_ / d_gcm_b_ hold the chunk rows
    void gcm_tag_tail(const uint64_t *d_a, size_t n_a, const uint64_t *d_b, size_t n_b, GcmCallPlan plan,
                      uint64_t *d_out_tagdiff);
    void gcm_square_pass(const uint64_t *d_src, size_t n_src, const std::vector<size_t> &blocks,
                         const std::vector<uint64_t *> &outs);
    void gcm_product_pass(const std::vector<const uint64_t *> &a, const std::vector<const uint64_t *> &b,
                          const std::vector<uint64_t *> &outs);
    // XTS: the refreshed tweaks of the call and the masks of the chunk in flight
    DevBuf<uint64_t> d_xts_tweaks_, d_xts_masks_;
    void xts_tweak_pass(const uint64_t *d_rk2, const uint8_t *d_tweaks, size_t n, int rounds, uint64_t *d_out, int nr);
    void copy_rows(const uint64_t *d_src, size_t src_stride, uint64_t *d_dst, size_t dst_stride, size_t rows,
                   size_t len);
    void copy_key_words(const uint64_t *d_src, size_t src_stride, uint64_t *d_dst, size_t dst_stride, size_t n_keys,
                        size_t len);
    // shortint_1bit: S-box / identity test vectors and tree-level scratch
    DevBuf<uint64_t> d_s1_sbox_tv_, d_s1_id_tv_, d_s1_in_, d_s1_out_, d_s1_pks_, d_s1_tv_;
    void require_s1() const;
    void cbs_vp_stages(const uint64_t *d_small_bits, size_t G, int n_in, const uint64_t *d_lut, int n_out,
                       uint64_t *d_out);
    // scratch
    DevBuf<uint64_t> d_small_, d_big_, d_ggsw_, d_state_, d_muls_;
    DevBuf<cplx> d_ggsw_f_;
    // stage timing (HIP events around each stage call on the engine stream, summed in collect_times)
    struct Span {
        hipEvent_t a, b;
        int stage;
    };
    size_t ev_used_ = 0;
    std::vector<Span> spans_;
    hipEvent_t next_event();
    template <class F>
    void timed(int stage, F fn);
    void collect_times();
    // int8 MFMA keyswitches (ksgemm.hpp): key limb matrices + digit scratch
    bool mfma_ks_ = false;
    // PFKS GEMM in the K layout (ksgemm.hpp KSlots) from pf_kl_min_ ciphertexts on, the 6-bit
    // row-tile limbs below (shorter K: 2.4x fewer K steps per tile, for batches too small to fill the
    // chip either way); TAE_PFKS_LAYOUT=k / rows forces one (the parity tests run both)
    bool pf_kl_ = false;
    long pf_kl_min_ = 2048;
    int kp_pf_kl_ = 0;
    ksgemm::KSlots pf_slots_;
    // K-layout GEMM kernel (TAE_PFKS_GEMM, read at init): 0 gemm_g6<6, 4, true>, 1.. the gemm_g7 variants;
    // default "w16" (8 waves of 96 x 128, 16x16x64 MFMAs), the fastest by stage and by bench wall time
    int pf_gemm_ = 3;
    const char *last_pfks_kernel_ = "none";
    DevBuf<int8_t> d_pf_bt_kl_;
    DevBuf<uint64_t> d_pf_corr_;   // [ncols] digit-offset correction of the K layout
    DevBuf<uint32_t> d_pf_flags_;  // [B][words] clamped-digit flags of the K layout (kslots_build)
    DevBuf<int8_t> d_pf_bt_, d_ks_bt_, d_digits_;
    int kp_pf_ = 0, kp_ks_ = 0;
    void prepare_mfma_keys();
    void pfks_keys(const uint64_t *d_big, size_t B, int q0, int nq, uint64_t *dst, long out_stride);
    void require_pack() const;
    DevBuf<uint64_t> d_pack_;  // pack_bits: keyswitch outputs of one chunk [bits][(k+1)N]
    // batched N=1024, k=2 blind rotation (br1024.hpp) for this set's (levels, base_log), or nullptr
    void (*br1024_pbs_)(const uint64_t *, int, const uint64_t *, int, const cplx *, int, uint64_t *, long, uint64_t,
                        uint64_t, const cplx *, const cplx *, const cplx *, const double *, uint64_t *) = nullptr;
    decltype(br1024_pbs_) br1024_vp_ = nullptr;
    decltype(br1024_pbs_) br1024_pbs1_ = nullptr;  // one ciphertext per workgroup (small batches)
    decltype(br1024_pbs_) br1024_occ2_ = nullptr;  // A/B: one per workgroup, two workgroups per CU
    int br1024_pbs1_lp_ = 1;                       // its levels per pass
    bool lf1k_ = false;                            // the 8-bit model's PBS: the N = 1024 fused transform (lf1k.hpp)
    bool b1kw_ = false;                            // ... on br1024w (four ciphertexts per workgroup, ACC stash)
    DevBuf<uint64_t> d_acc_w_;                     // br1024w's ACC stash [B][k+1][N]
    // latency blind rotation, one ciphertext per 1024-thread workgroup (br1024lat.hpp), or nullptr
    void (*br1024lat_)(const uint64_t *, int, const uint64_t *, const cplx *, uint64_t *, long, uint64_t, uint64_t,
                       const cplx *, const double *) = nullptr;
    size_t br1024lat_lds_ = 0;
    bool x4_512_ = false;     // PBS N = 512, k = 4, 3 x 2^12 (lvl_64): br512x4 / br512lat on the fused transform
    bool x4_vp_ = false;      // ... and cbs 1 x 2^13: vertical packing on br512x4<1, false, 13>
    bool lf512_ = false;      // N = 512, k = 4: the fused transform, conj(E2)-rescaled BSK (oracle lf_set)
    bool x4_s1_ = false;      // shortint_1bit PBS 7 x 2^6: br512x4<7, true, 6> with per-ciphertext test vectors
    long lat_max_ = 256;      // batch size up to which br512lat runs (TAE_BR_LAT_MAX)
    bool p16_ = false;        // lvl_64 PBS batches on br512p16 (two ciphertexts per workgroup) instead of br512x4
                              // (TAE_PBS_KERNEL = p16 / x4)
    int num_cu_ = 256;
    DevBuf<double> d_lf_;     // the fused-twiddle transform's table (lf512.hpp: params_sqrd_lvl_64, lf1k.hpp: 8-bit)
    bool timing_ = false, clock_ = false;
    DevBuf<uint64_t> d_clk_;
    uint64_t *clock_buffer(size_t wgs);                   // nullptr unless clock mode is on
    void record_clock(const uint64_t *clk, size_t wgs);  // median GHz of one stamped launch
    StageTimes times_;
};

}  // namespace tae
