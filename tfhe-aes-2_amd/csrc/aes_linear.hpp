// The linear layer of the forward cipher (AddRoundKey, ShiftRows, MixColumns) as LWE additions, one output word
// at a time: the forward counterpart of aes_inv.hpp.  The device kernels (aes_engine.hip) are grid-stride loops
// around these functions, so a host program runs the same arithmetic (tests/native/aes_linear_test.cpp).
//
// A state is [blk][16 bytes][8 bits][L] words (byte pos = 4*col + row, bits MSB first, L the LWE size); word t of
// it is coefficient `coef` of bit `bit` of byte `pos` of block `blk`.  The nullable arguments, the same in every
// function that has them:
//   map      the SubBytes output of (blk, byte) lies at group map[blk*16 + byte] (a counter plan's round 1,
//            ctr_plan.hpp) instead of at blk*16 + byte
//   key_of   multi-key batches: the round key of block blk is read at rk + key_of[blk] * key_stride,
//            the same round of slot key_of[blk] of a key table, instead of at rk.  The slot is uniform over the L
//            coefficients of a ciphertext, so the reads stay contiguous runs per wave.
// Each is null or not for a whole launch, so the branches on them are uniform.
#pragma once
#include <cstddef>
#include <cstdint>

#include "aes_inv.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TAE_LIN_HD __host__ __device__ inline
#else
#define TAE_LIN_HD inline
#endif

namespace tae {

struct AesWord {
    size_t coef, blk;
    int bit, pos;
};
TAE_LIN_HD AesWord aes_word(size_t t, int L) {
    const size_t ct = t / L;  // blk*128 + pos*8 + bit
    return {t % L, ct >> 7, (int)(ct & 7), (int)((ct >> 3) & 15)};
}

// after ShiftRows, element (row, c) comes from SubBytes output byte 4*((c+row)%4) + row
TAE_LIN_HD int shift_rows_src_byte(int row, int c) { return 4 * ((c + row) & 3) + row; }

TAE_LIN_HD size_t sub_bytes_group(const int32_t *map, size_t blk, int byte) {
    return map ? (size_t)map[blk * 16 + byte] : blk * 16 + byte;
}

TAE_LIN_HD const uint64_t *keyed_rk(const uint64_t *rk, const int32_t *key_of, size_t key_stride, size_t blk) {
    return key_of ? rk + (size_t)key_of[blk] * key_stride : rk;
}

// bit `bit` of a public byte as Context::trivial encodes it: << 63, to be added on the body (coef == L - 1)
TAE_LIN_HD uint64_t public_bit(int byte, int bit) { return (uint64_t)((byte >> (7 - bit)) & 1) << 63; }

// Round 0, and the inverse cipher's: word t of round key + input (xor_state, data_model.rs:270-274).  The input is
// the ciphertexts `blocks` [nb][128][L], the public `bytes` [nb*16] as trivial ciphertexts (CBC), both, or, with
// `groups` [U] = (pos << 8) | value, the deduplicated SubBytes inputs of a counter plan: state [U][8][L], group g
// under slot key_of[g] (the slot does not fit the 16-bit group word, so it is a parallel array).
TAE_LIN_HD uint64_t aes_round0_word(const uint64_t *rk, const uint64_t *blocks, const uint8_t *bytes,
                                    const uint16_t *groups, size_t t, int L, const int32_t *key_of, size_t key_stride) {
    const size_t coef = t % L, ct = t / L;
    const int bit = (int)(ct & 7);
    size_t owner = ct >> 7;  // whose slot: the block
    int pos = (int)((ct >> 3) & 15), value = bytes ? bytes[ct >> 3] : 0;
    if (groups) {
        owner = ct >> 3;  // the group
        pos = groups[owner] >> 8;
        value = groups[owner] & 0xff;
    }
    uint64_t w = keyed_rk(rk, key_of, key_stride, owner)[(size_t)(pos * 8 + bit) * L + coef];
    if (blocks) w += blocks[t];
    if (coef == (size_t)L - 1) w += public_bit(value, bit);
    return w;
}

// 1-bit model, a middle round: ShiftRows on the three SubBytes*{1,2,3} states muls [G][24][L], MixColumns,
// AddRoundKey: out[r][c] = 2s[r][c'] + s[r+3][.] + s[r+2][.] + 3s[r+1][.]  (fhe_sbox_gal_mul_pbs.rs:61-82)
TAE_LIN_HD uint64_t aes_mix_word(const uint64_t *muls, const int32_t *map, const uint64_t *rk_round, size_t t, int L,
                                 const int32_t *key_of, size_t key_stride) {
    const AesWord w = aes_word(t, L);
    const int c = w.pos >> 2, row = w.pos & 3;
    auto src = [&](int rr, int m) {
        const size_t g = sub_bytes_group(map, w.blk, shift_rows_src_byte(rr, c));
        return muls[((g * 24) + 8 * m + w.bit) * (size_t)L + w.coef];
    };
    return src(row, 1) + src((row + 3) & 3, 0) + src((row + 2) & 3, 0) + src((row + 1) & 3, 2) +
           keyed_rk(rk_round, key_of, key_stride, w.blk)[(size_t)(w.pos * 8 + w.bit) * L + w.coef];
}

// 8-bit and shortint_1bit models, a middle round: ShiftRows + MixColumns (fhe_sbox_pbs.rs:33-73: gf_256_mul as
// shifts and XORs of bits, i.e. LWE additions) + AddRoundKey on the SubBytes output sb [G][8][L].
// T.idx[o][*] = the input bits (column-local, byte-major, MSB-first, -1 terminated) summed into output bit o of
// a column (or_mix_column_terms in the oracle).
struct MixTerms {
    int8_t idx[32][8];
};
TAE_LIN_HD uint64_t aes8_mix_word(const uint64_t *sb, const int32_t *map, const uint64_t *rk_round, size_t t, int L,
                                  const MixTerms &T) {
    const AesWord w = aes_word(t, L);
    const int c = w.pos >> 2, o = 8 * (w.pos & 3) + w.bit;
    uint64_t acc = rk_round[(size_t)(w.pos * 8 + w.bit) * L + w.coef];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < 8; q++) {
        const int i = T.idx[o][q];
        if (i < 0) break;
        const size_t g = sub_bytes_group(map, w.blk, shift_rows_src_byte(i >> 3, c));
        acc += sb[(g * 8 + (i & 7)) * (size_t)L + w.coef];
    }
    return acc;
}

// The last round of either direction: word t of ShiftRows (inverse: InvShiftRows) of the SubBytes output
// sb [G][8][L] + the round key, stored at its place in `out`.  t runs over the first n_bytes bytes of the blocks
// in block order, n_bytes * 8 * L words.
//   data     public bytes, indexed like the output: bit b of data[i] is XORed into bit b of output byte i
//            (transciphering; CBC's previous ciphertext block)
//   blk_out, blk_len   several counter streams (CtrPlanMulti): block blk writes its first blk_len[blk] bytes at
//            byte blk_out[blk] of the concatenated output, instead of all 16 at byte 16 blk.  Every written
//            ciphertext is one contiguous run of L words.
TAE_LIN_HD void aes_final_word(const uint64_t *sb, const int32_t *map, const uint64_t *rk_round, const uint8_t *data,
                               uint64_t *out, size_t t, int L, const int32_t *key_of, size_t key_stride,
                               const int64_t *blk_out, const int32_t *blk_len, bool inverse) {
    const AesWord w = aes_word(t, L);
    if (blk_len && w.pos >= blk_len[w.blk]) return;
    const int c = w.pos >> 2, row = w.pos & 3;
    const int byte = inverse ? inv_final_src_byte(row, c) : shift_rows_src_byte(row, c);
    const size_t obyte = blk_out ? (size_t)blk_out[w.blk] + w.pos : w.blk * 16 + w.pos;
    uint64_t v = sb[(sub_bytes_group(map, w.blk, byte) * 8 + w.bit) * (size_t)L + w.coef] +
                 keyed_rk(rk_round, key_of, key_stride, w.blk)[(size_t)(w.pos * 8 + w.bit) * L + w.coef];
    if (data && w.coef == (size_t)L - 1) v += public_bit(data[obyte], w.bit);
    out[(obyte * 8 + w.bit) * (size_t)L + w.coef] = v;
}

}  // namespace tae
