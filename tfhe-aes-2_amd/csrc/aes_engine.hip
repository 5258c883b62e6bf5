// The AES application layer of the Engine: the linear layers between the circuit bootstraps as HIP kernels
// (ShiftRows / MixColumns / AddRoundKey as LWE additions: fhe_sbox_gal_mul_pbs.rs:61-132, data_model.rs:270-281;
// the arithmetic of a word is in aes_linear.hpp and aes_inv.hpp) and the drivers of every mode: the forward
// cipher on the three models, counter mode, the inverse cipher, CBC, XTS, CCM, GCM, multi-key batches and the two key
// derivations.  The generic TFHE stages they call are in kernels.hip.
#include <cstring>
#include <stdexcept>

#include "aes.hpp"
#include "aes_ccm.hpp"
#include "aes_gcm.hpp"
#include "aes_linear.hpp"
#include "aes_xts.hpp"
#include "engine_detail.hpp"
#include "rowsum.hpp"

namespace tae {

namespace {

// ---------------------------------------------------------------------------------------------
// Linear-layer kernels: consecutive threads walk the coefficients of one ciphertext, so every read and the
// write coalesce.  The nullable arguments are described in aes_linear.hpp.
// ---------------------------------------------------------------------------------------------
// state [n_cts][L] = round key + input: n_cts = nb * 128, or U * 8 with `groups`
__global__ void aes_round0_kernel(const uint64_t *__restrict__ rk, const uint64_t *__restrict__ blocks,
                                  const uint8_t *__restrict__ bytes, const uint16_t *__restrict__ groups,
                                  uint64_t *__restrict__ state, size_t n_cts, int L,
                                  const int32_t *__restrict__ key_of, size_t key_stride) {
    const size_t total = n_cts * (size_t)L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        state[t] = aes_round0_word(rk, blocks, bytes, groups, t, L, key_of, key_stride);
}

__global__ void aes_mix_kernel(const uint64_t *__restrict__ muls, const int32_t *__restrict__ map,
                               const uint64_t *__restrict__ rk_round, uint64_t *__restrict__ state, size_t nb, int L,
                               const int32_t *__restrict__ key_of, size_t key_stride) {
    const size_t total = nb * 128 * (size_t)L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        state[t] = aes_mix_word(muls, map, rk_round, t, L, key_of, key_stride);
}

__global__ void aes8_mix_kernel(const uint64_t *__restrict__ sb, const int32_t *__restrict__ map,
                                const uint64_t *__restrict__ rk_round, uint64_t *__restrict__ state, size_t nb, int L,
                                MixTerms T) {
    const size_t total = nb * 128 * (size_t)L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        state[t] = aes8_mix_word(sb, map, rk_round, t, L, T);
}

__global__ void aes_final_kernel(const uint64_t *__restrict__ sb, const int32_t *__restrict__ map,
                                 const uint64_t *__restrict__ rk_round, const uint8_t *__restrict__ data,
                                 uint64_t *__restrict__ out, size_t n_bytes, int L,
                                 const int32_t *__restrict__ key_of, size_t key_stride,
                                 const int64_t *__restrict__ blk_out, const int32_t *__restrict__ blk_len, bool inverse) {
    const size_t total = n_bytes * 8 * (size_t)L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        aes_final_word(sb, map, rk_round, data, out, t, L, key_of, key_stride, blk_out, blk_len, inverse);
}

// ---- AES-128 inverse cipher (FIPS-197 5.3; aes_inv.hpp has the algorithm and the source-byte indices) ----
// InvShiftRows (shift_rows != 0), InvMixColumns and AddRoundKey on the four InvSubBytes*{14,11,13,9} states:
// muls [nb*16][32][L], multiple m at ciphertexts 8m..8m+7 of a byte.  rk_round == nullptr adds no key and
// shift_rows == 0 skips InvShiftRows: InvMixColumns alone, which derives the decryption key from nb round keys.
__global__ void aes_inv_mix_kernel(const uint64_t *__restrict__ muls, const uint64_t *__restrict__ rk_round,
                                   uint64_t *__restrict__ state, size_t nb, int L, int shift_rows,
                                   const int32_t *__restrict__ key_of = nullptr, size_t key_stride = 0) {
    const size_t total = nb * 128 * (size_t)L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const AesWord w = aes_word(t, L);
        const int c = w.pos >> 2, row = w.pos & 3;
        uint64_t acc =
            rk_round ? keyed_rk(rk_round, key_of, key_stride, w.blk)[(size_t)(w.pos * 8 + w.bit) * L + w.coef] : 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int byte = inv_mix_src_byte(row, c, j, shift_rows != 0);
            acc += muls[(((w.blk * 16 + byte) * 32) + 8 * j + w.bit) * (size_t)L + w.coef];
        }
        state[t] = acc;
    }
}

// ---- row sums (rowsum.hpp): out [n_rows][L] from sources [n_src][L].  Consecutive lanes take consecutive
// coefficients of one output ciphertext.  Serves XTS's masks and GCM's squares, chunk sums, reductions and tag
// differences ----
__global__ void rowsum_kernel(const uint64_t *__restrict__ sources, const int32_t *__restrict__ row_start,
                              const int32_t *__restrict__ src, const int32_t *__restrict__ list_of,
                              const int32_t *__restrict__ base_of, const uint8_t *__restrict__ pub_bit,
                              uint64_t *__restrict__ out, size_t n_rows, int L) {
    const size_t total = n_rows * (size_t)L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        out[t] = rowsum_word(sources, row_start, src, list_of, base_of, pub_bit, t, L);
}

// the same over two source arrays (rowsum2_word): consecutive lanes on consecutive coefficients of one output
// ciphertext, and the array a source lies in is uniform over a row, so every read stays a contiguous run
__global__ void rowsum2_kernel(const uint64_t *__restrict__ A, size_t n_a, const uint64_t *__restrict__ B,
                               const int32_t *__restrict__ row_start, const int32_t *__restrict__ src,
                               const int32_t *__restrict__ list_of, const int32_t *__restrict__ base_of,
                               const uint8_t *__restrict__ pub_bit, uint64_t *__restrict__ out, size_t n_rows, int L) {
    const size_t total = n_rows * (size_t)L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        out[t] = rowsum2_word(A, n_a, B, row_start, src, list_of, base_of, pub_bit, t, L);
}

// ---- CCM (aes_ccm.hpp): the round-0 state [n][128][L] of a chain step from the previous cipher output x, the
// payload ciphertexts in the result buffer and the public bytes; the tag differences after the last step ----
__global__ void aes_ccm_absorb_kernel(const uint64_t *__restrict__ x, const uint64_t *__restrict__ plain,
                                      const uint64_t *__restrict__ rk, const int64_t *__restrict__ src,
                                      uint64_t *__restrict__ state, size_t n, int L, const int32_t *__restrict__ key_of,
                                      size_t key_stride, int nr) {
    const size_t total = n * 128 * (size_t)L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        state[t] = ccm_absorb_word(x, plain, rk, src, t, L, key_of, key_stride, nr);
}

__global__ void aes_ccm_tag_kernel(const uint64_t *__restrict__ x, const uint64_t *__restrict__ s0,
                                   const uint64_t *__restrict__ rk, const uint8_t *__restrict__ tags, int M,
                                   const int32_t *__restrict__ out_of, uint64_t *__restrict__ out, size_t n, int L,
                                   const int32_t *__restrict__ key_of, size_t key_stride, int nr) {
    const size_t total = n * 8 * (size_t)M * L;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
        ccm_tag_word(x, s0, rk, tags, M, out_of, out, t, L, key_of, key_stride, nr);
}

// ---- GCM (aes_gcm.hpp): the 1024 groups of `count` products from their keyswitched operand bits: small [count][256][S] (a's 128 bits, then
// b's) -> pairs [count][1024][8][S], input `bit` of group g being operand bit gcm_pair_source(g, bit)
__global__ void gcm_pairs_kernel(const uint64_t *__restrict__ small, uint64_t *__restrict__ pairs, size_t count, int S) {
    const size_t total = count * kGcmGroups * 8 * (size_t)S;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t coef = t % S, ct = t / S;
        const int bit = (int)(ct & 7), g = (int)((ct >> 3) & (kGcmGroups - 1));
        const size_t c = ct >> 13;
        pairs[t] = small[(c * 256 + (size_t)gcm_pair_source(g, bit)) * S + coef];
    }
}

// ---- AEAD open (aead_open.hpp): the groups of a verdict level or of a gate pass from small ciphertexts that were
// keyswitched once: out [n][S] = small [idx[t]][S], or the zero ciphertext where idx[t] < 0.  Consecutive lanes take
// consecutive coefficients of one output ciphertext; the host checks every index against the source count ----
__global__ void gather_small_kernel(const uint64_t *__restrict__ small, const int32_t *__restrict__ idx,
                                    uint64_t *__restrict__ out, size_t n, int S) {
    const size_t total = n * (size_t)S;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t ct = t / S, coef = t - ct * S;
        const int32_t s = idx[ct];
        out[t] = s < 0 ? 0 : small[(size_t)s * S + coef];
    }
}

// ---- key expansion (FIPS-197 5.2, figure 11): one word before its identity bootstrap ----
// t = back + other (+ Rcon), whole ciphertexts: back = rk[i-Nk], other = rk[i-1] or SubWord(rk[i-1]), both
// [4 bytes][8 bits][L].  SubWord works byte by byte, so RotWord is applied here, on the read of its output:
// rot = 1 takes byte (b + 1) % 4 of `other`.  rcon != 0 adds bit b of it (MSB first) << 63 on the body of bit b
// of byte 0, as Context::trivial does.  The same word of n_keys keys at once, key k reading
// back + k * back_stride and other + k * other_stride and writing out [n_keys][32][L].
__global__ void aes_ks_word_kernel(const uint64_t *__restrict__ back, const uint64_t *__restrict__ other, int rot,
                                   int rcon, uint64_t *__restrict__ out, int L, size_t n_keys, size_t back_stride,
                                   size_t other_stride) {
    const size_t word = 32 * (size_t)L, total = n_keys * word;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t key = t / word, within = t - key * word;
        const size_t coef = within % L;
        const int ct = (int)(within / L);  // byte*8 + bit
        const int bit = ct & 7, byte = ct >> 3;
        uint64_t w = back[key * back_stride + within] +
                     other[key * other_stride + (size_t)(((byte + rot) & 3) * 8 + bit) * L + coef];
        if (byte == 0 && coef == (size_t)L - 1) w += public_bit(rcon, bit);
        out[t] = w;
    }
}

// nr = 10 / 12 / 14 (AES-128 / 192 / 256) and 1 <= rounds <= nr, or a runtime_error
void require_rounds(int rounds, int nr) {
    if (nr != 10 && nr != 12 && nr != 14) throw std::runtime_error("the round count of the key size must be 10, 12 or 14");
    if (rounds < 1 || rounds > nr) throw std::runtime_error("rounds must be in 1..=" + std::to_string(nr));
}

// the two arrays every counter plan has, against its U groups and nb blocks
void check_ctr_plan(size_t U, const std::vector<int32_t> &map, size_t nb) {
    if (map.size() != nb * 16 || !U) throw std::runtime_error("counter plan does not match the blocks");
    for (int32_t g : map)
        if (g < 0 || (size_t)g >= U) throw std::runtime_error("counter plan: group index out of range");
}

}  // namespace

// Byte::bootstrap_with_lut of the 8-bit model: the circuit bootstrap into one 8-bit int per byte, then its bits
void Engine::bootstrap_bytes8(const uint64_t *d_bytes, size_t G, const uint64_t *d_lut, uint64_t *d_out) {
    if (!G) return;
    d_ints_.grow(G * p_.big_len());
    cbs_vp(d_bytes, G, 8, d_lut, 1, d_ints_);
    timed(ST_EXTRACT, [&] { extract_bits(d_ints_, G, 56, 8, d_out); });
    collect_times();
}

// ---------------------------------------------------------------------------------------------
// The forward cipher: one round loop for every model and mode
// ---------------------------------------------------------------------------------------------
// What a forward entry point asks of aes_forward.  Round 0 has the ciphertexts `blocks`, the public blocks `bytes`
// [nb*16] on the device (the XTS tweaks) or, with neither, the U deduplicated groups of a counter plan whose
// arrays are on the device (d_ctr_groups_, d_ctr_map_; the groups' slots in group_key).  `sub` is the model's SubBytes step.  The key slots and the output placement are
// aes_linear.hpp's nullable arguments.
struct Engine::AesRun {
    enum Sub { GAL_MUL, BYTES8, SHORTINT1 } sub;  // circuit_bootstrap 8 -> 24 / 8 -> 8, bootstrap_bytes8, s1_multivariate
    const uint64_t *rk;
    size_t nb;
    int rounds, nr;
    const uint64_t *blocks = nullptr;
    const uint8_t *bytes = nullptr;
    size_t U = 0;
    const int32_t *group_key = nullptr;
    const int32_t *key_of = nullptr;
    size_t key_stride = 0;
    bool time_linear = false;  // the linear launches are ST_LINEAR spans, collected at the end (keyed calls)
    const uint8_t *data = nullptr;
    size_t out_bytes = 0;  // the first out_bytes bytes of the blocks are written
    const int64_t *blk_out = nullptr;
    const int32_t *blk_len = nullptr;
    uint64_t *out = nullptr;
    // CCM.  state_ready: round 0 is in d_state_ already (a chain step's absorb kernel), nb blocks.  keep: the final
    // kernel runs a second time and places the same outputs at keep_out / keep_len of `keep` (no public bytes)
    bool state_ready = false;
    const int64_t *keep_out = nullptr;
    const int32_t *keep_len = nullptr;
    uint64_t *keep = nullptr;
};

// fhe_sbox_gal_mul_pbs::encrypt_block_for_rounds / fhe_sbox_pbs::encrypt_block_for_rounds over nb blocks.  Round 0
// leaves G groups of 8 bits in d_state_; each middle round is SubBytes of the G groups and the mix, which reads
// them through the plan's map once (round 1 of counter mode) and leaves 16 nb groups; the last SubBytes and the
// final kernel close the call.
void Engine::aes_forward(const AesRun &a) {
    const bool gal = a.sub == AesRun::GAL_MUL;
    const int L = (int)(gal ? p_.big_len() : p_.small_len());
    const size_t nb = a.nb, state_len = nb * 128 * (size_t)L, byte_stride = 8 * (size_t)L;
    const bool plan = !a.blocks && !a.bytes && !a.state_ready;
    size_t G = plan ? a.U : nb * 16;
    const int32_t *map = plan ? d_ctr_map_ : nullptr;
    // one round of a plan works on its U groups alone; the per-block state and the 24 SubBytes multiples of the
    // 1-bit model exist from round 2 on
    const bool groups_only = plan && a.rounds == 1;
    d_state_.grow(groups_only ? G * byte_stride : state_len);
    d_muls_.grow(groups_only ? G * byte_stride : nb * 16 * (gal ? 24 : 8) * (size_t)L);
    MixTerms T;
    std::memcpy(T.idx, mix_idx_, sizeof(T.idx));
    auto linear = [&](auto launch) {
        if (a.time_linear) {
            timed(ST_LINEAR, launch);
        } else {
            launch();
        }
    };
    auto sub_bytes = [&](bool last) {
        if (gal)
            circuit_bootstrap(d_state_, G, 8, last ? d_lut8_ : d_lut24_, last ? 8 : 24, d_muls_);
        else if (a.sub == AesRun::BYTES8)
            bootstrap_bytes8(d_state_, G, d_wlut_sbox_, d_muls_);
        else
            s1_multivariate(d_state_, G, 8, d_s1_sbox_tv_, 8, d_muls_);
    };
    if (!a.state_ready)
        linear([&] {
            aes_round0_kernel<<<grid_for(G * byte_stride), kThreads, 0, stream_>>>(
                a.rk, a.blocks, a.bytes, plan ? d_ctr_groups_ : nullptr, d_state_, G * 8, L,
                plan ? a.group_key : a.key_of, a.key_stride);
            HIPC(hipGetLastError());
        });
    for (int r = 1; r < a.rounds; r++) {
        sub_bytes(false);
        const uint64_t *rk_r = a.rk + (size_t)16 * r * byte_stride;
        linear([&] {
            if (gal)
                aes_mix_kernel<<<grid_for(state_len), kThreads, 0, stream_>>>(d_muls_, map, rk_r, d_state_, nb, L, a.key_of,
                                                                               a.key_stride);
            else
                aes8_mix_kernel<<<grid_for(state_len), kThreads, 0, stream_>>>(d_muls_, map, rk_r, d_state_, nb, L, T);
            HIPC(hipGetLastError());
        });
        G = nb * 16;
        map = nullptr;
    }
    sub_bytes(true);
    if (a.out_bytes)
        linear([&] {
            aes_final_kernel<<<grid_for(a.out_bytes * byte_stride), kThreads, 0, stream_>>>(
                d_muls_, map, a.rk + (size_t)16 * a.nr * byte_stride, a.data, a.out, a.out_bytes, L, a.key_of, a.key_stride,
                a.blk_out, a.blk_len, false);
            HIPC(hipGetLastError());
        });
    if (a.out_bytes && a.keep)
        linear([&] {
            aes_final_kernel<<<grid_for(a.out_bytes * byte_stride), kThreads, 0, stream_>>>(
                d_muls_, map, a.rk + (size_t)16 * a.nr * byte_stride, nullptr, a.keep, a.out_bytes, L, a.key_of,
                a.key_stride, a.keep_out, a.keep_len, false);
            HIPC(hipGetLastError());
        });
    if (a.time_linear) collect_times();
}

void Engine::aes_encrypt_blocks(const uint64_t *d_rk, const uint64_t *d_blocks, size_t nb, int rounds,
                                uint64_t *d_out, int nr, const int32_t *d_key_of, size_t key_stride) {
    if (!nb) return;
    require_rounds(rounds, nr);
    times_ = StageTimes{};
    AesRun a{AesRun::GAL_MUL, d_rk, nb, rounds, nr};
    a.blocks = d_blocks;
    a.key_of = d_key_of;
    a.key_stride = key_stride;
    a.time_linear = d_key_of != nullptr;  // the single-key path keeps its launches as they were: no event records
    a.out_bytes = nb * 16;
    a.out = d_out;
    aes_forward(a);
}

void Engine::aes8_encrypt_blocks(const uint64_t *d_rk, const uint64_t *d_blocks, size_t nb, int rounds,
                                 uint64_t *d_out) {
    if (!nb) return;
    if (p_.model != 8) throw std::runtime_error("aes8_encrypt_blocks needs the 8-bit model parameters");
    require_rounds(rounds, 10);
    times_ = StageTimes{};
    AesRun a{AesRun::BYTES8, d_rk, nb, rounds, 10};
    a.blocks = d_blocks;
    a.out_bytes = nb * 16;
    a.out = d_out;
    aes_forward(a);
}

// fhe_sbox_pbs::encrypt_block_for_rounds (fhe_sbox_pbs.rs:75-121) over nb blocks of shortint_1bit bits with
// ByteT::sbox_substitute = 8 multivariate functions per byte (fhe_impls/shortint_1bit.rs:32-50); MixColumns
// and AddRoundKey are the same LWE-addition network as the 8-bit model's (shortint unchecked_add,
// shortint_1bit.rs:109-120)
void Engine::s1_aes_encrypt_blocks(const uint64_t *d_rk, const uint64_t *d_blocks, size_t nb, int rounds,
                                   uint64_t *d_out) {
    require_s1();
    if (!nb) return;
    require_rounds(rounds, 10);
    times_ = StageTimes{};
    AesRun a{AesRun::SHORTINT1, d_rk, nb, rounds, 10};
    a.blocks = d_blocks;
    a.out_bytes = nb * 16;
    a.out = d_out;
    aes_forward(a);
    collect_times();  // the spans of s1_bootstrap
}

// ---- multi-key batches: a key table [n_keys][4 (nr + 1) * 32][L], block i under slot key_of[i] ----
// The uploads into the engine's buffers are asynchronous: the host array must live until the next call
const int32_t *Engine::upload_key_of(const int32_t *key_of, size_t nb) {
    key_of_host_.assign(key_of, key_of + nb);
    return d_key_of_.upload(key_of_host_.data(), nb, stream_);
}

void Engine::aes_encrypt_blocks_multi(const uint64_t *d_table, const int32_t *key_of, const uint64_t *d_blocks,
                                      size_t nb, int rounds, uint64_t *d_out, int nr) {
    if (!nb) return;
    if (p_.model != 1) throw std::runtime_error("multi-key batches need the 1-bit model parameters");
    require_rounds(rounds, nr);
    aes_encrypt_blocks(d_table, d_blocks, nb, rounds, d_out, nr, upload_key_of(key_of, nb),
                       (size_t)4 * (nr + 1) * 32 * p_.big_len());
}

// ---- AES-128-CTR with public counters (ctr_plan.hpp): round 1 runs on U deduplicated groups ----
// One chunk of a single-key call on the model of the parameter set: no input ciphertexts, the first out_bytes
// (<= 16 nb) keystream bytes, xor d_data if given
void Engine::aes_ctr_chunk(const uint64_t *d_rk, const CtrPlan &plan, size_t nb, int rounds, const uint8_t *d_data,
                           size_t out_bytes, uint64_t *d_out, int nr) {
    require_rounds(rounds, nr);
    if (out_bytes > nb * 16) throw std::runtime_error("more output bytes than keystream");
    check_ctr_plan(plan.groups.size(), plan.map, nb);
    d_ctr_groups_.upload(plan.groups.data(), plan.groups.size(), stream_);
    d_ctr_map_.upload(plan.map.data(), plan.map.size(), stream_);
    AesRun a{p_.model == 8 ? AesRun::BYTES8 : AesRun::GAL_MUL, d_rk, nb, rounds, nr};
    a.U = plan.groups.size();
    a.data = d_data;
    a.out_bytes = out_bytes;
    a.out = d_out;
    aes_forward(a);
}

void Engine::aes_ctr_blocks(const uint64_t *d_rk, const CtrPlan &plan, size_t nb, int rounds, const uint8_t *d_data,
                            size_t out_bytes, uint64_t *d_out, int nr) {
    if (!nb) return;
    if (p_.model != 1) throw std::runtime_error("aes_ctr_blocks needs the 1-bit model parameters");
    aes_ctr_chunk(d_rk, plan, nb, rounds, d_data, out_bytes, d_out, nr);
}

void Engine::aes8_ctr_blocks(const uint64_t *d_rk, const CtrPlan &plan, size_t nb, int rounds, const uint8_t *d_data,
                             size_t out_bytes, uint64_t *d_out, int nr) {
    if (!nb) return;
    if (p_.model != 8) throw std::runtime_error("aes8_ctr_blocks needs the 8-bit model parameters");
    aes_ctr_chunk(d_rk, plan, nb, rounds, d_data, out_bytes, d_out, nr);
}

void Engine::aes_ctr(const uint64_t *d_rk, const uint8_t iv[8], uint64_t first_counter, size_t nb, int rounds,
                     const uint8_t *d_data, size_t out_bytes, uint64_t *d_out, int nr) {
    if (!nb) return;
    if (p_.model != 1 && p_.model != 8) throw std::runtime_error("counter mode runs on the 1-bit and 8-bit models");
    if (!ctr_range_ok(first_counter, nb)) throw std::runtime_error("counter range wraps past 2^64 - 1");
    if (out_bytes > nb * 16) throw std::runtime_error("more output bytes than keystream");
    times_ = StageTimes{};
    const size_t L = p_.bit_len();
    // the uploads of a plan are asynchronous: every chunk's plan lives until the next call
    ctr_plans_.clear();
    ctr_plans_.reserve((nb + ctr_chunk_ - 1) / ctr_chunk_);
    for (size_t b0 = 0; b0 < nb; b0 += ctr_chunk_) {
        const size_t cn = std::min(ctr_chunk_, nb - b0);
        const size_t byte0 = b0 * 16;
        const size_t cbytes = out_bytes > byte0 ? std::min(cn * 16, out_bytes - byte0) : 0;
        ctr_plans_.emplace_back();
        ctr_plan(iv, first_counter + b0, cn, ctr_plans_.back());
        const uint8_t *data = d_data ? d_data + byte0 : nullptr;
        uint64_t *out = d_out + byte0 * 8 * L;
        aes_ctr_chunk(d_rk, ctr_plans_.back(), cn, rounds, data, cbytes, out, nr);
    }
}

// One chunk of a multi-stream call: the round keys of every block and group are read from their slot of the key
// table, and the final kernel writes each block's bytes at its place in the concatenated output
void Engine::aes_ctr_blocks_multi(const uint64_t *d_table, const CtrPlanMulti &plan, int rounds, const uint8_t *d_data,
                                  uint64_t *d_out, int nr, const std::vector<int64_t> *keep_out,
                                  const std::vector<int32_t> *keep_len, uint64_t *d_keep) {
    const size_t nb = plan.block_slot.size(), U = plan.groups.size();
    if (!nb) return;
    if (plan.group_slot.size() != U || plan.block_out.size() != nb || plan.block_len.size() != nb)
        throw std::runtime_error("counter plan does not match the blocks");
    if (d_keep && (!keep_out || !keep_len || keep_out->size() != nb || keep_len->size() != nb))
        throw std::runtime_error("counter plan: the second placement does not match the blocks");
    check_ctr_plan(U, plan.map, nb);
    // a block that only the second placement takes has length 0 in the first
    for (size_t i = 0; i < nb; i++) {
        const int32_t n = plan.block_len[i], k = d_keep ? (*keep_len)[i] : 0;
        if (n < (k ? 0 : 1) || n > 16 || (k != 0 && k != 16))
            throw std::runtime_error("counter plan: block length out of range");
    }
    d_ctr_groups_.upload(plan.groups.data(), U, stream_);
    d_ctr_map_.upload(plan.map.data(), nb * 16, stream_);
    AesRun a{AesRun::GAL_MUL, d_table, nb, rounds, nr};
    a.U = U;
    a.group_key = d_ctr_gslot_.upload(plan.group_slot.data(), U, stream_);
    a.key_of = d_key_of_.upload(plan.block_slot.data(), nb, stream_);
    a.key_stride = (size_t)4 * (nr + 1) * 32 * p_.big_len();
    a.time_linear = true;
    a.data = d_data;
    a.out_bytes = nb * 16;
    a.blk_out = d_ctr_bout_.upload(plan.block_out.data(), nb, stream_);
    a.blk_len = d_ctr_blen_.upload(plan.block_len.data(), nb, stream_);
    a.out = d_out;
    if (d_keep) {
        a.keep_out = d_pub_kout_.upload(keep_out->data(), nb, stream_);
        a.keep_len = d_pub_klen_.upload(keep_len->data(), nb, stream_);
        a.keep = d_keep;
    }
    aes_forward(a);
}

void Engine::aes_ctr_multi(const uint64_t *d_table, const std::vector<CtrBlock> &blocks, int rounds,
                           const uint8_t *d_data, uint64_t *d_out, int nr) {
    if (blocks.empty()) return;
    if (p_.model != 1) throw std::runtime_error("multi-key batches need the 1-bit model parameters");
    require_rounds(rounds, nr);
    times_ = StageTimes{};
    // the uploads of a plan are asynchronous: every chunk's plan lives until the next call.  A chunk boundary may
    // fall inside a stream: a block carries its slot, counter and output place with it.
    ctr_mplans_.clear();
    ctr_mplans_.reserve((blocks.size() + ctr_chunk_ - 1) / ctr_chunk_);
    for (size_t b0 = 0; b0 < blocks.size(); b0 += ctr_chunk_) {
        const size_t cn = std::min(ctr_chunk_, blocks.size() - b0);
        ctr_mplans_.emplace_back();
        ctr_plan_multi(blocks.data() + b0, cn, ctr_mplans_.back());
        aes_ctr_blocks_multi(d_table, ctr_mplans_.back(), rounds, d_data, d_out, nr);
    }
}

// ---------------------------------------------------------------------------------------------
// AES-CCM decryption of public frames (aes_ccm.hpp)
// ---------------------------------------------------------------------------------------------
void Engine::pub_pass(const uint64_t *d_table, const std::vector<PubBlock> &blocks, int rounds, const uint8_t *d_data,
                      uint64_t *d_out, int nr, const std::vector<int64_t> *keep_out, const std::vector<int32_t> *keep_len,
                      uint64_t *d_keep) {
    // the uploads of a plan are asynchronous: every chunk's plan and lists live until the next pass
    const size_t n_chunks = (blocks.size() + ctr_chunk_ - 1) / ctr_chunk_;
    ctr_mplans_.clear();
    pub_kout_.clear();
    pub_klen_.clear();
    ctr_mplans_.reserve(n_chunks);
    pub_kout_.reserve(n_chunks);
    pub_klen_.reserve(n_chunks);
    for (size_t b0 = 0; b0 < blocks.size(); b0 += ctr_chunk_) {
        const size_t cn = std::min(ctr_chunk_, blocks.size() - b0);
        ctr_mplans_.emplace_back();
        pub_plan(blocks.data() + b0, cn, ctr_mplans_.back());
        if (!d_keep) {
            aes_ctr_blocks_multi(d_table, ctr_mplans_.back(), rounds, d_data, d_out, nr);
            continue;
        }
        pub_kout_.emplace_back(keep_out->begin() + b0, keep_out->begin() + b0 + cn);
        pub_klen_.emplace_back(keep_len->begin() + b0, keep_len->begin() + b0 + cn);
        aes_ctr_blocks_multi(d_table, ctr_mplans_.back(), rounds, d_data, d_out, nr, &pub_kout_.back(), &pub_klen_.back(),
                             d_keep);
    }
}

void Engine::aes_pub_blocks_multi(const uint64_t *d_table, const std::vector<PubBlock> &blocks, int rounds,
                                  uint64_t *d_out, int nr) {
    if (blocks.empty()) return;
    if (p_.model != 1) throw std::runtime_error("multi-key batches need the 1-bit model parameters");
    require_rounds(rounds, nr);
    times_ = StageTimes{};
    pub_pass(d_table, blocks, rounds, nullptr, d_out, nr);
}

void Engine::aes_ccm_transcipher(const uint64_t *d_table, const std::vector<CcmStreamIn> &streams, int rounds, int nr,
                                 uint64_t *d_out_plain, uint64_t *d_out_tagdiff) {
    const size_t n = streams.size();
    if (!n) return;
    if (p_.model != 1) throw std::runtime_error("CCM runs on the 1-bit model parameters");
    require_rounds(rounds, nr);
    // at one round the de-duplicated SubBytes outputs of B_0 and A_0 coincide at the nonce positions, and the tag
    // difference would add a ciphertext to itself
    if (rounds < 2) throw std::runtime_error("CCM needs rounds >= 2");
    const int M = streams[0].frame->M, L = (int)p_.big_len();
    const size_t block_len = 128 * (size_t)L, key_stride = (size_t)4 * (nr + 1) * 32 * L;
    std::vector<int64_t> off(n);  // the first payload byte of every frame in the result
    size_t total = 0;
    for (size_t s = 0; s < n; s++) {
        const CcmFrame &f = *streams[s].frame;
        if (f.M != M || !f.n_mac() || f.n_ctr() != 1 + (f.payload_len + 15) / 16 || f.src.size() != f.mac.size())
            throw std::runtime_error("CCM frames of one call have one tag length and a whole layout");
        off[s] = (int64_t)total;
        total += f.payload_len;
    }
    times_ = StageTimes{};
    // the chain order: by decreasing MAC-block count, so the streams of a step are a prefix
    ccm_order_.resize(n);
    for (size_t s = 0; s < n; s++) ccm_order_[s] = (int32_t)s;
    std::stable_sort(ccm_order_.begin(), ccm_order_.end(), [&](int32_t a, int32_t b) {
        return streams[(size_t)a].frame->n_mac() > streams[(size_t)b].frame->n_mac();
    });
    std::vector<size_t> rank(n);
    ccm_slot_.resize(n);
    ccm_bytes_.assign(total + n * (size_t)M, 0);  // the payload ciphertexts in result order, then the tags in chain order
    for (size_t j = 0; j < n; j++) {
        const CcmStreamIn &st = streams[(size_t)ccm_order_[j]];
        rank[(size_t)ccm_order_[j]] = j;
        ccm_slot_[j] = st.slot;
        if (st.frame->payload_len)
            std::memcpy(&ccm_bytes_[(size_t)off[(size_t)ccm_order_[j]]], st.data, st.frame->payload_len);
        std::memcpy(&ccm_bytes_[total + j * (size_t)M], st.tag, (size_t)M);
    }
    const uint8_t *d_bytes = d_ccm_bytes_.upload(ccm_bytes_.data(), ccm_bytes_.size(), stream_);
    const int32_t *d_slot = d_ccm_slot_.upload(ccm_slot_.data(), n, stream_);
    const int32_t *d_order = d_ccm_order_.upload(ccm_order_.data(), n, stream_);
    d_ccm_keep_.grow(2 * n * block_len);
    uint64_t *d_s0 = d_ccm_keep_, *d_x = d_ccm_keep_ + n * block_len;  // chain order, both

    // ---- pass 1: A_1 .. A_n into the result, A_0 and B_0 into the kept blocks ----
    std::vector<PubBlock> blocks;
    std::vector<int64_t> kout;
    std::vector<int32_t> klen;
    auto add = [&](int32_t slot, const uint8_t *bytes, int64_t out_byte, int32_t len, int64_t keep_byte) {
        PubBlock b;
        b.slot = slot;
        std::memcpy(b.bytes, bytes, 16);
        b.out_byte = out_byte;
        b.len = len;
        blocks.push_back(b);
        kout.push_back(keep_byte < 0 ? 0 : keep_byte);
        klen.push_back(keep_byte < 0 ? 0 : 16);
    };
    for (size_t s = 0; s < n; s++) {
        const CcmFrame &f = *streams[s].frame;
        for (size_t i = 1; i < f.n_ctr(); i++)
            add(streams[s].slot, &f.ctr[16 * i], off[s] + (int64_t)(16 * (i - 1)),
                (int32_t)std::min<size_t>(16, f.payload_len - 16 * (i - 1)), -1);
        add(streams[s].slot, &f.ctr[0], 0, 0, (int64_t)(16 * rank[s]));
        add(streams[s].slot, &f.mac[0], 0, 0, (int64_t)(16 * (n + rank[s])));
    }
    pub_pass(d_table, blocks, rounds, d_bytes, d_out_plain, nr, &kout, &klen, d_ccm_keep_);

    // ---- the chain: step t absorbs MAC block t of the streams that have one ----
    auto mac_blocks = [&](size_t j) { return streams[(size_t)ccm_order_[j]].frame->n_mac(); };
    const size_t depth = mac_blocks(0);
    std::vector<size_t> step_at(depth, 0), step_n(depth, 0);
    ccm_src_.clear();
    for (size_t t = 1; t < depth; t++) {
        step_at[t] = ccm_src_.size();
        for (size_t j = 0; j < n && mac_blocks(j) > t; j++) {
            const size_t s = (size_t)ccm_order_[j];
            const CcmFrame &f = *streams[s].frame;
            for (int pos = 0; pos < 16; pos++) {
                const int64_t q = f.src[t * 16 + pos];
                ccm_src_.push_back(q >= 0 ? off[s] + q : ccm_src_public(f.mac[t * 16 + pos]));
            }
            step_n[t] = j + 1;
        }
    }
    const int64_t *d_src = ccm_src_.empty() ? nullptr : d_ccm_src_.upload(ccm_src_.data(), ccm_src_.size(), stream_);
    if (depth > 1) d_state_.grow(step_n[1] * block_len);  // the largest step: aes_forward keeps the buffer
    for (size_t t = 1; t < depth; t++) {
        const size_t na = step_n[t];
        timed(ST_LINEAR, [&] {
            aes_ccm_absorb_kernel<<<grid_for(na * block_len), kThreads, 0, stream_>>>(
                d_x, d_out_plain, d_table, d_src + step_at[t], d_state_, na, L, d_slot, key_stride, nr);
            HIPC(hipGetLastError());
        });
        AesRun a{AesRun::GAL_MUL, d_table, na, rounds, nr};
        a.state_ready = true;
        a.key_of = d_slot;
        a.key_stride = key_stride;
        a.time_linear = true;
        a.out_bytes = na * 16;
        a.out = d_x;
        aes_forward(a);
    }
    timed(ST_LINEAR, [&] {
        aes_ccm_tag_kernel<<<grid_for(n * 8 * (size_t)M * L), kThreads, 0, stream_>>>(
            d_x, d_s0, d_table, d_bytes + total, M, d_order, d_out_tagdiff, n, L, d_slot, key_stride, nr);
        HIPC(hipGetLastError());
    });
    collect_times();
}

// ---------------------------------------------------------------------------------------------
// AES-GCM decryption of public frames (aes_gcm.hpp)
// ---------------------------------------------------------------------------------------------
void Engine::require_gcm() const {
    if (p_.model != 1 || !d_lut_gcm_ || !d_lut_id1_) throw std::runtime_error("GCM runs on the 1-bit model parameters");
}

// Row sums (rowsum.hpp) for GCM and XTS: one launch, rowsum_kernel over A alone or rowsum2_kernel over A and B.  The
// plan's arrays are uploaded asynchronously into buffers the stream's earlier launches may still read, which the stream
// order allows; the host copy lives until the next call clears rowsum_plans_.
void Engine::rowsum_pass(const uint64_t *d_a, size_t n_a, const uint64_t *d_b, size_t n_b, RowPlan plan,
                         uint64_t *d_out) {
    if (!rowplan2_ok(plan, n_a, n_b)) throw std::runtime_error("row-sum plan: index out of range");
    if (!plan.n_rows()) return;
    rowsum_plans_.push_back(std::move(plan));
    const RowPlan &p = rowsum_plans_.back();
    auto up = [&](auto &d_buf, const auto &v) {  // an empty array is a null argument
        return v.empty() ? nullptr : d_buf.upload(v.data(), v.size(), stream_);
    };
    const int32_t *rs = up(d_rs_start_, p.row_start), *ix = up(d_rs_src_, p.src);
    const int32_t *lo = up(d_rs_list_, p.list_of), *bo = up(d_rs_base_, p.base_of);
    const uint8_t *pb = up(d_rs_pub_, p.pub_bit);
    const int L = (int)p_.big_len();
    const size_t n_rows = p.n_rows();
    const unsigned grid = grid_for(n_rows * (size_t)L);
    timed(ST_LINEAR, [&] {
        if (n_b)
            rowsum2_kernel<<<grid, kThreads, 0, stream_>>>(d_a, n_a, d_b, rs, ix, lo, bo, pb, d_out, n_rows, L);
        else
            rowsum_kernel<<<grid, kThreads, 0, stream_>>>(d_a, rs, ix, lo, bo, pb, d_out, n_rows, L);
        HIPC(hipGetLastError());
    });
}

// Squares of blocks `blocks` of the source array [n_src / 128][128][L], square s written to outs[s]: one row-sum
// launch and one identity bootstrap for all of them
void Engine::gcm_square_pass(const uint64_t *d_src, size_t n_src, const std::vector<size_t> &blocks,
                             const std::vector<uint64_t *> &outs) {
    const size_t n = blocks.size(), block_len = 128 * p_.big_len();
    if (!n) return;
    RowPlan plan = gcm_square_plan();  // the one list set, read at every operand's base
    for (size_t s = 0; s < n; s++)
        for (int32_t r = 0; r < 128; r++) {
            plan.list_of.push_back(r);
            plan.base_of.push_back((int32_t)(blocks[s] * 128));
        }
    d_gcm_a_.grow(n * block_len);
    d_gcm_b_.grow(n * block_len);
    rowsum_pass(d_src, n_src, std::move(plan), d_gcm_a_);
    circuit_bootstrap(d_gcm_a_, n * 128, 1, d_lut_id1_, 1, d_gcm_b_);
    for (size_t s = 0; s < n; s++)
        HIPC(hipMemcpyAsync(outs[s], d_gcm_b_ + s * block_len, block_len * 8, hipMemcpyDeviceToDevice, stream_));
}

// Products a[c] b[c] -> outs[c], each [128][L].  Keyswitching after a gather of big ciphertexts would run 8192
// keyswitches per product for the same words: the keyswitch is per ciphertext, so the 256 operand bits go through it
// once and the small ciphertexts are gathered.
void Engine::gcm_product_pass(const std::vector<const uint64_t *> &a, const std::vector<const uint64_t *> &b,
                              const std::vector<uint64_t *> &outs) {
    const size_t n = a.size(), L = p_.big_len(), S = p_.small_len(), block_len = 128 * L;
    if (!n) return;
    const GcmProductPlan one = gcm_product_plan();
    const size_t n_chunks = one.chunks.n_rows();
    // a product's plan once, product c reading its sources at c * stride
    auto per_product = [n](RowPlan p, size_t stride) {
        const size_t n_lists = p.n_lists();
        for (size_t r = 0; r < n * n_lists; r++) {
            p.list_of.push_back((int32_t)(r % n_lists));
            p.base_of.push_back((int32_t)(r / n_lists * stride));
        }
        return p;
    };
    d_gcm_ops_.grow(n * 2 * block_len);
    d_gcm_ks_.grow(n * 256 * S);
    d_gcm_parts_.grow(n * kGcmParts * L);
    d_gcm_a_.grow(n * n_chunks * L);
    d_gcm_b_.grow(n * n_chunks * L);
    for (size_t c = 0; c < n; c++) {
        HIPC(hipMemcpyAsync(d_gcm_ops_ + 2 * c * block_len, a[c], block_len * 8, hipMemcpyDeviceToDevice, stream_));
        HIPC(hipMemcpyAsync(d_gcm_ops_ + (2 * c + 1) * block_len, b[c], block_len * 8, hipMemcpyDeviceToDevice, stream_));
    }
    timed(ST_KS, [&] { keyswitch(d_gcm_ops_, d_gcm_ks_, n * 256); });
    // the groups are written where cbs_vp's own reserve leaves its scratch: reserved first, so the buffer stays
    reserve(n * kGcmGroups * 8, n * kGcmParts);
    timed(ST_LINEAR, [&] {
        gcm_pairs_kernel<<<grid_for(n * kGcmGroups * 8 * S), kThreads, 0, stream_>>>(d_gcm_ks_, d_small_, n, (int)S);
        HIPC(hipGetLastError());
    });
    cbs_vp(d_small_, n * kGcmGroups, 8, d_lut_gcm_, kGcmPartBits, d_gcm_parts_);
    rowsum_pass(d_gcm_parts_, n * kGcmParts, per_product(one.chunks, kGcmParts), d_gcm_a_);
    circuit_bootstrap(d_gcm_a_, n * n_chunks, 1, d_lut_id1_, 1, d_gcm_b_);
    rowsum_pass(d_gcm_b_, n * n_chunks, per_product(one.reduce, n_chunks), d_gcm_a_);
    circuit_bootstrap(d_gcm_a_, n * 128, 1, d_lut_id1_, 1, d_gcm_b_);
    for (size_t c = 0; c < n; c++)
        HIPC(hipMemcpyAsync(outs[c], d_gcm_b_ + c * block_len, block_len * 8, hipMemcpyDeviceToDevice, stream_));
}

void Engine::gf128_square(const uint64_t *d_in, size_t count, uint64_t *d_out) {
    require_gcm();
    if (!count) return;
    times_ = StageTimes{};
    rowsum_plans_.clear();
    const size_t block_len = 128 * p_.big_len();
    std::vector<size_t> blocks(count);
    std::vector<uint64_t *> outs(count);
    for (size_t c = 0; c < count; c++) {
        blocks[c] = c;
        outs[c] = d_out + c * block_len;
    }
    gcm_square_pass(d_in, count * 128, blocks, outs);
    collect_times();
}

void Engine::gf128_product(const uint64_t *d_a, const uint64_t *d_b, size_t count, uint64_t *d_out) {
    require_gcm();
    if (!count) return;
    times_ = StageTimes{};
    rowsum_plans_.clear();
    const size_t block_len = 128 * p_.big_len();
    std::vector<const uint64_t *> a(count), b(count);
    std::vector<uint64_t *> outs(count);
    for (size_t c = 0; c < count; c++) {
        a[c] = d_a + c * block_len;
        b[c] = d_b + c * block_len;
        outs[c] = d_out + c * block_len;
    }
    gcm_product_pass(a, b, outs);
    collect_times();
}

// Power k of a table's base at its entry k - 1: a generation's squares of all tables in one launch sequence, its
// products in another.  The product scratch grows with the batch, so several tables split a generation's products at
// gcm_seg_batch_; the bootstraps are per ciphertext, so where a batch ends changes no word.
void Engine::gcm_power_generations(uint64_t *d_base, size_t n_blocks, const std::vector<size_t> &tabs, int n) {
    const size_t block_len = 128 * p_.big_len();
    for (const GcmGeneration &gen : gcm_power_schedule(n)) {
        std::vector<size_t> blocks;
        std::vector<const uint64_t *> a, b;
        std::vector<uint64_t *> sq_out, pr_out;
        for (size_t t0 : tabs) {
            uint64_t *d_tab = d_base + t0 * block_len;
            for (int k : gen.squares) {
                blocks.push_back(t0 + (size_t)(k / 2 - 1));
                sq_out.push_back(d_tab + (size_t)(k - 1) * block_len);
            }
            for (int k : gen.products) {
                a.push_back(d_tab + (size_t)(k - 2) * block_len);
                b.push_back(d_tab);
                pr_out.push_back(d_tab + (size_t)(k - 1) * block_len);
            }
        }
        gcm_square_pass(d_base, n_blocks * 128, blocks, sq_out);
        const size_t batch = tabs.size() > 1 ? gcm_seg_batch_ : std::max<size_t>(a.size(), 1);
        for (size_t at = 0; at < a.size(); at += batch) {
            const size_t end = std::min(a.size(), at + batch);
            gcm_product_pass({a.begin() + (std::ptrdiff_t)at, a.begin() + (std::ptrdiff_t)end},
                             {b.begin() + (std::ptrdiff_t)at, b.begin() + (std::ptrdiff_t)end},
                             {pr_out.begin() + (std::ptrdiff_t)at, pr_out.begin() + (std::ptrdiff_t)end});
        }
    }
}

// The power tables of a key table; a single key is a table of one slot.  H = E_K(0^128) of every slot comes out of one
// public-block batch and one identity bootstrap (H^1 at noise^2 = 1) in slot order; a row copy puts it at entry 0 of the
// slot's table, and the generations run over all tables.
void Engine::ghash_key_multi(const uint64_t *d_table, size_t n_keys, int n_powers, int rounds, int nr, uint64_t *d_out) {
    require_gcm();
    require_rounds(rounds, nr);
    if (n_powers < 1 || n_powers > kGcmMaxPowers) throw std::runtime_error("GCM: n_powers must be in 1..=64");
    if (!gcm_multi_shape_ok(n_keys, (size_t)n_powers, 0)) throw std::runtime_error("GCM: too many keys for one call");
    if (!n_keys) return;
    const size_t block_len = 128 * p_.big_len();
    rowsum_plans_.clear();
    std::vector<PubBlock> zeros(n_keys);
    std::vector<size_t> tabs(n_keys);
    for (size_t s = 0; s < n_keys; s++) {
        zeros[s] = PubBlock{};
        zeros[s].slot = (int32_t)s;
        zeros[s].out_byte = (int64_t)(16 * s);
        zeros[s].len = 16;
        tabs[s] = s * (size_t)n_powers;
    }
    d_gcm_a_.grow(n_keys * block_len);
    d_gcm_b_.grow(n_keys * block_len);
    aes_pub_blocks_multi(d_table, zeros, rounds, d_gcm_a_, nr);  // resets the stage times
    circuit_bootstrap(d_gcm_a_, n_keys * 128, 1, d_lut_id1_, 1, d_gcm_b_);
    copy_rows(d_gcm_b_, block_len, d_out, (size_t)n_powers * block_len, n_keys, block_len);
    gcm_power_generations(d_out, n_keys * (size_t)n_powers, tabs, n_powers);
    collect_times();
}

void Engine::ghash_stride_key(const uint64_t *d_hk, size_t n_powers, size_t seg, int n_strides, uint64_t *d_out) {
    require_gcm();
    if (seg < 1 || seg > n_powers || seg > (size_t)kGcmMaxPowers)
        throw std::runtime_error("GCM: seg must be in 1..=min(n_powers, 64)");
    if (n_strides < 1 || n_strides > kGcmMaxStrides) throw std::runtime_error("GCM: n_strides must be in 1..=64");
    const size_t block_len = 128 * p_.big_len();
    times_ = StageTimes{};
    rowsum_plans_.clear();
    HIPC(hipMemcpyAsync(d_out, d_hk + (seg - 1) * block_len, block_len * 8, hipMemcpyDeviceToDevice, stream_));
    gcm_power_generations(d_out, (size_t)n_strides, {0}, n_strides);
    collect_times();
}

size_t Engine::gcm_frame_offsets(const std::vector<GcmFrameIn> &frames, std::vector<int64_t> &off) const {
    const int tag_len = frames[0].frame->tag_len;
    size_t total = 0;
    off.resize(frames.size());
    for (size_t s = 0; s < frames.size(); s++) {
        const GcmFrame &f = *frames[s].frame;
        if (f.tag_len != tag_len || !f.m() || f.n_pub() != 2 + (f.data_len + 15) / 16)
            throw std::runtime_error("GCM frames of one call have one tag length and a whole layout");
        off[s] = (int64_t)total;
        total += f.data_len;
    }
    return total;
}

void Engine::gcm_public_pass(const uint64_t *d_table, const std::vector<GcmFrameIn> &frames,
                             const std::vector<int64_t> &off, size_t total, int rounds, int nr, uint64_t *d_out_plain,
                             uint64_t *d_j0) {
    const size_t n = frames.size();
    gcm_bytes_.assign(std::max<size_t>(total, 1), 0);
    for (size_t s = 0; s < n; s++)
        if (frames[s].frame->data_len) std::memcpy(&gcm_bytes_[(size_t)off[s]], frames[s].data, frames[s].frame->data_len);
    const uint8_t *d_bytes = d_gcm_bytes_.upload(gcm_bytes_.data(), gcm_bytes_.size(), stream_);
    // the counters into the result, J0 into the kept blocks
    std::vector<PubBlock> blocks;
    std::vector<int64_t> kout;
    std::vector<int32_t> klen;
    for (size_t s = 0; s < n; s++) {
        const GcmFrame &f = *frames[s].frame;
        for (size_t i = 1; i < f.n_pub(); i++) {
            PubBlock b{};
            b.slot = frames[s].slot;
            std::memcpy(b.bytes, &f.pub[16 * i], 16);
            const bool j0 = i == 1;
            b.out_byte = j0 ? 0 : off[s] + (int64_t)(16 * (i - 2));
            b.len = j0 ? 0 : (int32_t)std::min<size_t>(16, f.data_len - 16 * (i - 2));
            blocks.push_back(b);
            kout.push_back(j0 ? (int64_t)(16 * s) : 0);
            klen.push_back(j0 ? 16 : 0);
        }
    }
    pub_pass(d_table, blocks, rounds, d_bytes, d_out_plain, nr, &kout, &klen, d_j0);
}

// GHASH + E(J0) + the received tag: chunk sums over A and B, one refresh, the differences
void Engine::gcm_tag_tail(const uint64_t *d_a, size_t n_a, const uint64_t *d_b, size_t n_b, GcmCallPlan plan,
                          uint64_t *d_out_tagdiff) {
    const size_t n_chunks = plan.chunks.n_rows();
    rowsum_pass(d_a, n_a, d_b, n_b, std::move(plan.chunks), d_gcm_a_);
    circuit_bootstrap(d_gcm_a_, n_chunks, 1, d_lut_id1_, 1, d_gcm_b_);
    rowsum_pass(d_gcm_b_, n_chunks, std::move(plan.diff), d_out_tagdiff);
}

// The short-frame call.  A is the caller's power tables where they lie, B the kept E(J0)
// blocks in d_gcm_src_: nothing of a table is copied.  Frame s under slot t reads its table at base 128 t n_powers and
// bit r of its E(J0) at source (n_keys n_powers + s) 128 + r.
void Engine::gcm_frames_pass(const uint64_t *d_table, size_t n_keys, const uint64_t *d_htable, size_t n_powers,
                             const std::vector<GcmFrameIn> &frames, int rounds, int nr, uint64_t *d_out_plain,
                             uint64_t *d_out_tagdiff) {
    const size_t n = frames.size();
    if (!n) return;
    require_gcm();
    require_rounds(rounds, nr);
    // at one round J0 and the counter blocks share their de-duplicated SubBytes outputs at the IV positions
    if (rounds < 2) throw std::runtime_error("GCM needs rounds >= 2");
    if (!gcm_plan_index_ok(n_keys, n_powers, n)) throw std::runtime_error("GCM: more sources than a row-sum index takes");
    const size_t L = p_.big_len(), block_len = 128 * L;
    // ---- the plans, before any device work ----
    std::vector<int64_t> off;
    const size_t total = gcm_frame_offsets(frames, off);  // one tag length, whole layouts
    GcmCallPlan plan;
    std::vector<std::vector<int32_t>> rows;
    for (size_t s = 0; s < n; s++) {
        const GcmFrame &f = *frames[s].frame;
        gcm_frame_rows(f, rows);
        switch (gcm_multi_frame_check(f, frames[s].slot, n_keys, n_powers, frames[0].frame->tag_len, rows)) {
            case GCM_MULTI_OK: break;
            case GCM_MULTI_SLOT: throw std::runtime_error("GCM frame: key slot outside 0..n_keys-1");
            default: throw std::runtime_error("GCM frame: more hashed blocks than the power table or the chunk sum takes");
        }
        gcm_multi_plan_add(plan, rows, n_keys, n_powers, (size_t)frames[s].slot, s, frames[s].tag);
    }
    const size_t n_a = n_keys * n_powers * 128, n_b = n * 128, n_chunks = plan.chunks.n_rows();
    if (!rowplan2_ok(plan.chunks, n_a, n_b)) throw std::runtime_error("row-sum plan: index out of range");
    times_ = StageTimes{};
    rowsum_plans_.clear();
    d_gcm_src_.grow(n * block_len);
    d_gcm_a_.grow(n_chunks * L);
    d_gcm_b_.grow(n_chunks * L);
    gcm_public_pass(d_table, frames, off, total, rounds, nr, d_out_plain, d_gcm_src_);
    gcm_tag_tail(d_htable, n_a, d_gcm_src_, n_b, std::move(plan), d_out_tagdiff);
    collect_times();
}

void Engine::aes_gcm_transcipher(const uint64_t *d_rk, const uint64_t *d_hk, size_t n_powers,
                                 const std::vector<GcmFrameIn> &frames, int rounds, int nr, uint64_t *d_out_plain,
                                 uint64_t *d_out_tagdiff) {
    gcm_frames_pass(d_rk, 1, d_hk, n_powers, frames, rounds, nr, d_out_plain, d_out_tagdiff);
}

// The key-table door's own bound comes before the shared checks (the model, where the status codes are made, refuses
// all of them first; only this backstop's message for a call with two reasons to refuse depends on the order)
void Engine::aes_gcm_transcipher_multi(const uint64_t *d_table, size_t n_keys, const uint64_t *d_htable, size_t n_powers,
                                       const std::vector<GcmFrameIn> &frames, int rounds, int nr, uint64_t *d_out_plain,
                                       uint64_t *d_out_tagdiff) {
    if (!frames.empty() && !gcm_multi_shape_ok(n_keys, n_powers, frames.size()))
        throw std::runtime_error("GCM: n_powers must be in 1..=64");
    gcm_frames_pass(d_table, n_keys, d_htable, n_powers, frames, rounds, nr, d_out_plain, d_out_tagdiff);
}

// Segmented GHASH (aes_gcm.hpp).  The plans index the table's first table_blocks powers, E(J0) of
// every frame, then every product S_c G_c; the table is read where d_hk keeps it, and d_gcm_src_ is sized once and
// holds, in blocks of [128][K+1], the rest and one batch of S_c operands.
// gcm_product_pass grows d_gcm_a_ / d_gcm_b_ / d_gcm_ops_ before it copies its operands, so no operand lives in those:
// S_c is written into d_gcm_src_ and the stride operands are read from the caller's d_sk.
void Engine::aes_gcm_long_transcipher(const uint64_t *d_rk, const uint64_t *d_hk, size_t n_powers, const uint64_t *d_sk,
                                      size_t n_strides, size_t seg, const std::vector<GcmFrameIn> &frames, int rounds,
                                      int nr, uint64_t *d_out_plain, uint64_t *d_out_tagdiff) {
    const size_t n = frames.size();
    if (!n) return;
    require_gcm();
    require_rounds(rounds, nr);
    if (rounds < 2) throw std::runtime_error("GCM needs rounds >= 2");
    const size_t L = p_.big_len(), block_len = 128 * L, B = gcm_seg_batch_;
    // ---- the plans, before any device work ----
    std::vector<int64_t> off;
    const size_t total = gcm_frame_offsets(frames, off);
    size_t table_blocks = 0, n_products = 0;
    std::vector<size_t> first_product(n);
    for (size_t s = 0; s < n; s++) {
        const size_t m = frames[s].frame->m();
        if (gcm_long_shape_check(m, seg, n_powers, n_strides) != GCM_LONG_OK)
            throw std::runtime_error("GCM: seg must be in 1..=n_powers and a frame's segments need a stride power each");
        table_blocks = std::max(table_blocks, std::min(seg, m));
        first_product[s] = n_products;
        n_products += gcm_long_segments(m, seg) - 1;
    }
    const size_t prod_block0 = table_blocks + n;  // in the plans' index space: table blocks, E(J0), products
    std::vector<GcmInnerPlan> inner((n_products + B - 1) / B);
    std::vector<size_t> stride_of;  // [n_products]: the stride power (c - 1) of every inner segment, in call order
    GcmCallPlan plan;
    std::vector<std::vector<int32_t>> rows;
    for (size_t s = 0; s < n; s++) {
        const GcmFrame &f = *frames[s].frame;
        for (size_t c = 1; c < gcm_long_segments(f.m(), seg); c++) {
            gcm_segment_rows(f, seg, c, 128, rows);
            if (!gcm_inner_rows_ok(rows)) throw std::runtime_error("GCM frame: an inner row needs more than 64 chunks");
            gcm_inner_plan_add(inner[stride_of.size() / B], rows);
            stride_of.push_back(c - 1);
        }
        gcm_long_final_rows(f, seg, prod_block0 + first_product[s], rows);
        if (!gcm_final_rows_ok(rows)) throw std::runtime_error("GCM frame: a tag row needs more than 64 chunks");
        gcm_call_plan_add(plan, rows, table_blocks, s, frames[s].tag);
    }
    // A = the table's first table_blocks blocks where the caller keeps them (seg <= n_powers backs them); B = d_gcm_src_
    const size_t n_a = table_blocks * 128, n_b = (n + n_products) * 128;
    const size_t n_chunks = plan.chunks.n_rows(), batch = std::min(B, n_products);
    size_t scratch = std::max(n_chunks, batch * gcm_product_plan().chunks.n_rows());
    for (const GcmInnerPlan &ip : inner) scratch = std::max(scratch, ip.chunks.n_rows());
    times_ = StageTimes{};
    rowsum_plans_.clear();
    d_gcm_src_.grow((n + n_products + batch) * block_len);
    d_gcm_a_.grow(scratch * L);
    d_gcm_b_.grow(scratch * L);
    gcm_public_pass(d_rk, frames, off, total, rounds, nr, d_out_plain, d_gcm_src_);

    // ---- the inner segments: S_c at level 1 with fresh ids, then S_c G_c behind the E(J0) blocks ----
    uint64_t *d_prod = d_gcm_src_ + n * block_len, *d_s = d_prod + n_products * block_len;
    for (size_t bi = 0; bi < inner.size(); bi++) {
        const size_t at = bi * B, nb = std::min(B, n_products - at), nck = inner[bi].chunks.n_rows();
        rowsum_pass(d_hk, n_a, std::move(inner[bi].chunks), d_gcm_a_);
        circuit_bootstrap(d_gcm_a_, nck, 1, d_lut_id1_, 1, d_gcm_b_);
        rowsum_pass(d_gcm_b_, nck, std::move(inner[bi].rows), d_gcm_a_);
        circuit_bootstrap(d_gcm_a_, nb * 128, 1, d_lut_id1_, 1, d_s);
        std::vector<const uint64_t *> a(nb), b(nb);
        std::vector<uint64_t *> outs(nb);
        for (size_t j = 0; j < nb; j++) {
            a[j] = d_s + j * block_len;
            b[j] = d_sk + stride_of[at + j] * block_len;
            outs[j] = d_prod + (at + j) * block_len;
        }
        gcm_product_pass(a, b, outs);
    }

    // ---- GHASH + E(J0) + the received tag, as the short-frame call: the products are sources like the table's ----
    gcm_tag_tail(d_hk, n_a, d_gcm_src_, n_b, std::move(plan), d_out_tagdiff);
    collect_times();
}

// ---------------------------------------------------------------------------------------------
// AEAD open: the verdict bit and the gated payload (aead_open.hpp).  Both keep their keyswitched
// ciphertexts in d_gcm_ks_ and the verdict its level outputs in d_gcm_a_; the groups are gathered into d_small_, where
// cbs_vp's own reserve leaves its scratch (reserved first, as gcm_product_pass does).  The keyswitch is per ciphertext,
// so a gathered small ciphertext has the words the keyswitch of the gathered big one would have, and the all-zero big
// ciphertext keyswitches to the all-zero small one: body 0, and every digit of a zero mask is 0.
// ---------------------------------------------------------------------------------------------
namespace {
void require_open(const Params &p) {
    if (p.model != 1) throw std::runtime_error("the AEAD open runs on the 1-bit model parameters");
}

// every entry of an index table is -1 or below n_src
void check_gather(const std::vector<int32_t> &idx, size_t n_src) {
    for (int32_t s : idx)
        if (s < -1 || (s >= 0 && (size_t)s >= n_src)) throw std::runtime_error("AEAD open: gather index out of range");
}
}  // namespace

void Engine::aead_verdict(const uint64_t *d_tag_diff, const VerdictPlan &plan, const std::vector<const int32_t *> &d_idx,
                          const uint64_t *d_lut_or8, const uint64_t *d_lut_nor8, uint64_t *d_ok) {
    require_open(p_);
    const size_t n = plan.n_frames, L = p_.big_len(), S = p_.small_len();
    const int levels = plan.levels();
    if (!n) return;
    if (levels < 1 || d_idx.size() != (size_t)levels) throw std::runtime_error("AEAD open: the plan has no levels");
    for (int l = 0; l < levels; l++) {
        if (plan.idx[l].size() != n * plan.groups[l] * kOpenOrBits || (l && plan.bits[l] != plan.groups[l - 1]))
            throw std::runtime_error("AEAD open: the verdict plan does not match its frames");
        check_gather(plan.idx[l], n * plan.bits[l]);
    }
    if (plan.groups[levels - 1] != 1) throw std::runtime_error("AEAD open: the last verdict level has one group");
    d_gcm_ks_.grow(n * plan.bits[0] * S);
    d_gcm_a_.grow(n * plan.groups[0] * L);
    reserve(n * plan.groups[0] * kOpenOrBits, n * plan.groups[0]);
    timed(ST_KS, [&] { keyswitch(d_tag_diff, d_gcm_ks_, n * plan.bits[0]); });
    for (int l = 0; l < levels; l++) {
        const bool last = l + 1 == levels;
        const size_t G = n * plan.groups[l];
        timed(ST_LINEAR, [&] {
            gather_small_kernel<<<grid_for(G * kOpenOrBits * S), kThreads, 0, stream_>>>(d_gcm_ks_, d_idx[l], d_small_,
                                                                                         G * kOpenOrBits, (int)S);
            HIPC(hipGetLastError());
        });
        cbs_vp(d_small_, G, kOpenOrBits, last ? d_lut_nor8 : d_lut_or8, 1, last ? d_ok : d_gcm_a_.get());
        if (!last) timed(ST_KS, [&] { keyswitch(d_gcm_a_, d_gcm_ks_, G); });
    }
    collect_times();
}

void Engine::aead_gate(const uint64_t *d_plain, const GatePlan &plan, const std::vector<const int32_t *> &d_idx,
                       const uint64_t *d_ok, const uint64_t *d_lut_gate, uint64_t *d_out) {
    require_open(p_);
    const size_t n_bytes = plan.n_bytes(), n = plan.n_frames, L = p_.big_len(), S = p_.small_len();
    const size_t pass = aead_gate_pass();
    if (!n_bytes) return;
    if (d_idx.size() != (n_bytes + pass - 1) / pass) throw std::runtime_error("AEAD open: one index table per gate pass");
    for (int32_t f : plan.frame_of_byte)
        if (f < 0 || (size_t)f >= n) throw std::runtime_error("AEAD open: frame index out of range");
    const size_t widest = std::min(pass, n_bytes);
    d_gcm_ks_.grow((n + widest * 8) * S);
    reserve(widest * kOpenGateBits, widest * 8);
    // the verdicts go through the keyswitch once and are copied into the byte groups as small ciphertexts
    timed(ST_KS, [&] { keyswitch(d_ok, d_gcm_ks_, n); });
    for (size_t g0 = 0, i = 0; g0 < n_bytes; g0 += pass, i++) {
        const size_t m = std::min(pass, n_bytes - g0);
        timed(ST_KS, [&] { keyswitch(d_plain + g0 * 8 * L, d_gcm_ks_ + n * S, m * 8); });
        timed(ST_LINEAR, [&] {
            gather_small_kernel<<<grid_for(m * kOpenGateBits * S), kThreads, 0, stream_>>>(d_gcm_ks_, d_idx[i], d_small_,
                                                                                           m * kOpenGateBits, (int)S);
            HIPC(hipGetLastError());
        });
        cbs_vp(d_small_, m, kOpenGateBits, d_lut_gate, 8, d_out + g0 * 8 * L);
    }
    collect_times();
}

// ---------------------------------------------------------------------------------------------
// AES inverse cipher (FIPS-197 5.3; aes_inv.hpp)
// ---------------------------------------------------------------------------------------------
void Engine::require_inverse(int rounds, int nr) const {
    if (p_.model != 1 || !d_lut_inv32_) throw std::runtime_error("the inverse cipher needs the 1-bit model parameters");
    require_rounds(rounds, nr);
}

// Round 0 on the ciphertexts d_blocks, on the public blocks d_cur or on both (XTS: the masks and C), rounds
// R-1 .. 1 and the last round, which XORs the public blocks d_xor in if given: R circuit bootstraps per block.
// keep_times: the stage times add to those of the call's earlier passes.
void Engine::aes_decrypt_rounds(const uint64_t *d_dk, const uint64_t *d_blocks, const uint8_t *d_cur, size_t nb,
                                int rounds, const uint8_t *d_xor, uint64_t *d_out, int nr, const int32_t *d_key_of,
                                size_t key_stride, bool keep_times) {
    const int L = (int)p_.big_len();
    const size_t state_len = nb * 128 * (size_t)L, byte_stride = 8 * (size_t)L;
    if (!keep_times) times_ = StageTimes{};
    d_state_.grow(state_len);
    d_muls_.grow(nb * 16 * (size_t)(rounds > 1 ? 32 : 8) * L);
    timed(ST_LINEAR, [&] {
        aes_round0_kernel<<<grid_for(state_len), kThreads, 0, stream_>>>(d_dk + (size_t)16 * nr * byte_stride, d_blocks,
                                                                          d_cur, nullptr, d_state_, nb * 128, L, d_key_of,
                                                                          key_stride);
        HIPC(hipGetLastError());
    });
    for (int r = rounds - 1; r >= 1; r--) {
        circuit_bootstrap(d_state_, nb * 16, 8, d_lut_inv32_, 32, d_muls_);
        timed(ST_LINEAR, [&] {
            aes_inv_mix_kernel<<<grid_for(state_len), kThreads, 0, stream_>>>(d_muls_, d_dk + (size_t)16 * r * byte_stride,
                                                                               d_state_, nb, L, 1, d_key_of, key_stride);
            HIPC(hipGetLastError());
        });
    }
    circuit_bootstrap(d_state_, nb * 16, 8, d_lut_inv8_, 8, d_muls_);
    timed(ST_LINEAR, [&] {
        aes_final_kernel<<<grid_for(state_len), kThreads, 0, stream_>>>(d_muls_, nullptr, d_dk, d_xor, d_out, nb * 16, L,
                                                                         d_key_of, key_stride, nullptr, nullptr, true);
        HIPC(hipGetLastError());
    });
    collect_times();
}

void Engine::aes_decrypt_blocks(const uint64_t *d_dk, const uint64_t *d_blocks, size_t nb, int rounds,
                                uint64_t *d_out, int nr, const int32_t *d_key_of, size_t key_stride) {
    if (!nb) return;
    require_inverse(rounds, nr);
    aes_decrypt_rounds(d_dk, d_blocks, nullptr, nb, rounds, nullptr, d_out, nr, d_key_of, key_stride);
}

void Engine::aes_decrypt_blocks_multi(const uint64_t *d_dtable, const int32_t *key_of, const uint64_t *d_blocks,
                                      size_t nb, int rounds, uint64_t *d_out, int nr) {
    if (!nb) return;
    require_inverse(rounds, nr);
    aes_decrypt_blocks(d_dtable, d_blocks, nb, rounds, d_out, nr, upload_key_of(key_of, nb),
                       (size_t)4 * (nr + 1) * 32 * p_.big_len());
}

void Engine::aes_cbc_transcipher(const uint64_t *d_dk, const uint8_t *d_iv_data, size_t nb, int rounds,
                                 uint64_t *d_out, int nr) {
    if (!nb) return;
    require_inverse(rounds, nr);
    // d_iv_data = iv || C_0 .. C_{nb-1}: block i is decrypted from bytes 16 (i + 1) .. and XORed with bytes 16 i ..
    aes_decrypt_rounds(d_dk, nullptr, d_iv_data + 16, nb, rounds, d_iv_data, d_out, nr, nullptr, 0);
}

// d_cur / d_prev [nb][16]: the ciphertext block and the block before it (the stream's iv for its first block)
void Engine::aes_cbc_transcipher_multi(const uint64_t *d_dtable, const int32_t *key_of, const uint8_t *d_cur,
                                       const uint8_t *d_prev, size_t nb, int rounds, uint64_t *d_out, int nr) {
    if (!nb) return;
    require_inverse(rounds, nr);
    aes_decrypt_rounds(d_dtable, nullptr, d_cur, nb, rounds, d_prev, d_out, nr, upload_key_of(key_of, nb),
                       (size_t)4 * (nr + 1) * 32 * p_.big_len());
}

// ---------------------------------------------------------------------------------------------
// XTS-AES decryption of a public ciphertext (aes_xts.hpp)
// ---------------------------------------------------------------------------------------------
// T = Enc_K2(tweak) for n public tweaks: the forward cipher on public blocks, left in d_state_, and one identity
// bootstrap of the 128 n bits, which brings every tweak bit to noise^2 = 1 whatever the unit size
void Engine::xts_tweak_pass(const uint64_t *d_rk2, const uint8_t *d_tweaks, size_t n, int rounds, uint64_t *d_out,
                            int nr) {
    AesRun a{AesRun::GAL_MUL, d_rk2, n, rounds, nr};
    a.bytes = d_tweaks;
    a.time_linear = true;
    a.out_bytes = n * 16;
    // the final kernel reads d_muls_ and the key alone, so the state buffer is free to take the cipher's output
    a.out = d_state_.grow(n * 128 * p_.big_len());
    aes_forward(a);
    circuit_bootstrap(d_state_, n * 128, 1, d_lut_id1_, 1, d_out);
}

void Engine::aes_xts_tweaks(const uint64_t *d_rk2, const uint8_t *d_tweaks, size_t n, int rounds, uint64_t *d_out,
                            int nr) {
    if (!n) return;
    require_inverse(rounds, nr);
    times_ = StageTimes{};
    xts_tweak_pass(d_rk2, d_tweaks, n, rounds, d_out, nr);
}

void Engine::aes_xts_masks(const uint64_t *d_tweak_cts, size_t n_units, const RowPlan &plan, uint64_t *d_masks) {
    if (!plan.n_rows()) return;
    if (p_.model != 1) throw std::runtime_error("XTS runs on the 1-bit model parameters");
    // a mask sums bits of its own unit's tweak: rowsum_pass bounds base + src, which alone would let a row reach
    // into the next unit
    for (int32_t s : plan.src)
        if (s > 127) throw std::runtime_error("XTS plan: source ciphertext out of range");
    for (int32_t b : plan.base_of)
        if (b % 128) throw std::runtime_error("XTS plan: unit or row-list index out of range");
    times_ = StageTimes{};
    rowsum_plans_.clear();
    rowsum_pass(d_tweak_cts, n_units * 128, plan, d_masks);
    collect_times();
}

void Engine::aes_xts_transcipher(const uint64_t *d_dk1, const uint64_t *d_rk2, const uint8_t *d_tweaks, size_t n_tweaks,
                                 const int32_t *tweak_of, const uint64_t *block_index, const uint8_t *d_data, size_t nb,
                                 int rounds, uint64_t *d_out, int nr) {
    if (!nb) return;
    require_inverse(rounds, nr);
    const size_t block_len = 128 * p_.big_len();
    times_ = StageTimes{};
    d_xts_tweaks_.grow(n_tweaks * block_len);
    xts_tweak_pass(d_rk2, d_tweaks, n_tweaks, rounds, d_xts_tweaks_, nr);
    // the tweaks stay resident across the chunks; every chunk's plan lives until the next call
    rowsum_plans_.clear();
    d_xts_masks_.grow(std::min(ctr_chunk_, nb) * block_len);
    for (size_t b0 = 0; b0 < nb; b0 += ctr_chunk_) {
        const size_t cn = std::min(ctr_chunk_, nb - b0);
        uint64_t *out = d_out + b0 * block_len;
        rowsum_pass(d_xts_tweaks_, n_tweaks * 128, xts_plan(tweak_of + b0, block_index + b0, cn), d_xts_masks_);
        aes_decrypt_rounds(d_dk1, d_xts_masks_, d_data + b0 * 16, cn, rounds, nullptr, out, nr, nullptr, 0, true);
        timed(ST_LINEAR, [&] { lwe_add(out, d_xts_masks_, cn * block_len); });
    }
    collect_times();
}

// ---------------------------------------------------------------------------------------------
// Key derivations on a key table [n_keys][W*32][L].  A table of one key is contiguous: its words
// are read and bootstrapped where they lie, and nothing is gathered or scattered.
// ---------------------------------------------------------------------------------------------
void Engine::copy_rows(const uint64_t *d_src, size_t src_stride, uint64_t *d_dst, size_t dst_stride, size_t rows,
                       size_t len) {
    timed(ST_LINEAR, [&] {
        copy_rows_strided_kernel<<<grid_for(rows * len), kThreads, 0, stream_>>>(d_src, src_stride, d_dst, dst_stride,
                                                                                  rows, len);
        HIPC(hipGetLastError());
    });
}

// `len` words at the same place of every key: an asynchronous copy for one key (none in place), a row copy for more
void Engine::copy_key_words(const uint64_t *d_src, size_t src_stride, uint64_t *d_dst, size_t dst_stride, size_t n_keys,
                            size_t len) {
    if (n_keys > 1)
        copy_rows(d_src, src_stride, d_dst, dst_stride, n_keys, len);
    else if (d_src != d_dst)
        HIPC(hipMemcpyAsync(d_dst, d_src, len * 8, hipMemcpyDeviceToDevice, stream_));
}

void Engine::aes_decrypt_key(const uint64_t *d_rk, uint64_t *d_dk, int nr) {
    require_inverse(nr, nr);
    if (d_rk == d_dk) throw std::runtime_error("the decryption key cannot be derived in place");
    aes_decrypt_key_multi(d_rk, 1, d_dk, nr);
}

void Engine::aes_decrypt_key_multi(const uint64_t *d_table, size_t n_keys, uint64_t *d_dtable, int nr) {
    require_inverse(nr, nr);
    if (d_table == d_dtable) throw std::runtime_error("the decryption keys cannot be derived in place");
    if (!n_keys) return;
    const int L = (int)p_.big_len();
    // words 4 .. 4 nr - 1: nr - 1 round keys of 16 bytes
    const size_t word = 32 * (size_t)L, mid = 4 * (size_t)(nr - 1) * word, last = 4 * (size_t)nr * word;
    const size_t stride = last + 4 * word;
    const bool one = n_keys == 1;
    times_ = StageTimes{};
    d_state_.grow(n_keys * mid);
    d_muls_.grow(n_keys * 16 * (size_t)(nr - 1) * 32 * L);
    copy_key_words(d_table, stride, d_dtable, stride, n_keys, 4 * word);
    copy_key_words(d_table + last, stride, d_dtable + last, stride, n_keys, 4 * word);
    const uint64_t *middle = d_table + 4 * word;
    if (!one) {
        copy_rows(middle, stride, d_state_, mid, n_keys, mid);
        middle = d_state_;
    }
    circuit_bootstrap(middle, n_keys * 16 * (size_t)(nr - 1), 8, d_lut_mul32_, 32, d_muls_);
    timed(ST_LINEAR, [&] {
        aes_inv_mix_kernel<<<grid_for(n_keys * mid), kThreads, 0, stream_>>>(d_muls_, nullptr, d_state_,
                                                                              n_keys * (size_t)(nr - 1), L, 0);
        HIPC(hipGetLastError());
    });
    circuit_bootstrap(d_state_, n_keys * 128 * (size_t)(nr - 1), 1, d_lut_id1_, 1, one ? d_dtable + 4 * word : d_muls_);
    if (!one) copy_rows(d_muls_, mid, d_dtable + 4 * word, stride, n_keys, mid);
    collect_times();
}

void Engine::aes_key_expand(const uint64_t *d_key, int nk, uint64_t *d_rk) { aes_key_expand_multi(d_key, nk, 1, d_rk); }

// Key expansion (FIPS-197 5.2, figure 11), nk = 4 / 6 / 8 key words, word i of all keys at once: the bootstraps
// of a word run over n_keys times the bits, so the number of chained circuit bootstraps is that of one key.
// Every new word is bootstrapped (identity, 32 one-bit groups per key) before the next word reads it, as
// Context::aes_key_schedule does on the host; the stages of a word are launches on the engine stream and no
// ciphertext leaves the device.  The table is key-major: for several keys, word i - 1 of every key is gathered
// for SubWord and the bootstrapped word scattered into the table rows.
void Engine::aes_key_expand_multi(const uint64_t *d_keys, int nk, size_t n_keys, uint64_t *d_table) {
    if (p_.model != 1 || !d_lut_id1_) throw std::runtime_error("the key expansion needs the 1-bit model parameters");
    if (nk != 4 && nk != 6 && nk != 8) throw std::runtime_error("the key must be 4, 6 or 8 words");
    if (!n_keys) return;
    const int L = (int)p_.big_len(), words = 4 * (nk + 7);
    const size_t word = 32 * (size_t)L, stride = (size_t)words * word, batch = n_keys * word;
    const bool one = n_keys == 1;
    times_ = StageTimes{};
    d_state_.grow(batch);
    d_muls_.grow(batch);
    copy_key_words(d_keys, (size_t)nk * word, d_table, stride, n_keys, (size_t)nk * word);
    for (int i = nk; i < words; i++) {
        const uint64_t *back = d_table + (size_t)(i - nk) * word, *other = d_table + (size_t)(i - 1) * word;
        size_t other_stride = stride;
        int rot = 0, rcon = 0;
        if (i % nk == 0 || (nk == 8 && i % 8 == 4)) {
            // SubWord of rk[i-1]; RotWord and Rcon on the words that start a key-sized group
            if (!one) {
                copy_rows(other, stride, d_state_, word, n_keys, word);
                other = d_state_;
            }
            circuit_bootstrap(other, 4 * n_keys, 8, d_lut8_, 8, d_muls_);
            other = d_muls_;
            other_stride = word;
            if (i % nk == 0) {
                rot = 1;
                rcon = kRcon[i / nk];
            }
        }
        timed(ST_LINEAR, [&] {
            aes_ks_word_kernel<<<grid_for(batch), kThreads, 0, stream_>>>(back, other, rot, rcon, d_state_, L, n_keys,
                                                                           stride, other_stride);
            HIPC(hipGetLastError());
        });
        uint64_t *dst = d_table + (size_t)i * word;
        circuit_bootstrap(d_state_, 32 * n_keys, 1, d_lut_id1_, 1, one ? dst : d_muls_);
        if (!one) copy_rows(d_muls_, word, dst, stride, n_keys, word);
    }
    collect_times();
}

}  // namespace tae
