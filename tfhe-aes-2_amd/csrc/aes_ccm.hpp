// AES-CCM (RFC 3610 / NIST SP 800-38C) decryption of a public frame under FHE: the host side and the arithmetic
// of the chain's linear step.  Plain C++: the formatting and the plan have no device code, and the
// two word functions are host/device like aes_linear.hpp's, so a stand-alone program runs them
// (tests/native/aes_ccm_test.cpp).
//
// A frame is (nonce of 15 - L bytes, AAD, ciphertext of the payload || U, the M-byte encrypted tag).  With
// S_i = E(A_i), A_i = (L-1) || nonce || be_L(i):  payload block i is C_i ^ S_i (i >= 1), the CBC-MAC runs over
// B_0 || encoded AAD || zero-padded payload, X_0 = E(B_0), X_t = E(X_{t-1} ^ B_t), and the frame is authentic iff
// the first M bytes of X_last ^ S_0 ^ U are zero.  The server sees neither the payload nor that difference: it
// returns both under FHE and the client compares.
//
// Every A_i and B_0 is public, so they go through the forward cipher as one batch of public blocks (pub_plan, the
// (slot, pos, value) de-duplication of ctr_plan.hpp on arbitrary blocks).  The chain is sequential: step t builds
// the cipher's round-0 state of every stream that still has a MAC block from the previous output and the block's
// bytes, which are public (B_0's successors in the AAD, the padding) or payload (the plaintext ciphertexts the
// first pass left in the result buffer).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "aes_linear.hpp"
#include "ctr_plan.hpp"

namespace tae {

// ---- formatting (RFC 3610 section 2) ----
struct CcmFrame {
    int L = 0, M = 0;             // bytes of the length field (2..8) and of the tag (4, 6 .. 16)
    size_t aad_len = 0, payload_len = 0;
    std::vector<uint8_t> ctr;     // [1 + ceil(payload_len / 16)][16]: A_0, A_1 ..
    std::vector<uint8_t> mac;     // [n_mac][16]: the public bytes of the MAC blocks, 0 where a payload byte goes
    std::vector<int64_t> src;     // [n_mac][16]: -1 = public (mac has the value), else the index of the payload byte
    size_t n_ctr() const { return ctr.size() / 16; }
    size_t n_mac() const { return mac.size() / 16; }
};

enum CcmFormat { CCM_FMT_OK = 0, CCM_FMT_NONCE, CCM_FMT_TAG, CCM_FMT_AAD, CCM_FMT_LEN };

// The longest AAD of the two-byte length form (RFC 3610: 0 < l(a) < 2^16 - 2^8)
constexpr size_t kCcmAadLimit = 0xFF00;

// On an error the frame is left empty.  nonce_len 7..13 (L = 15 - nonce_len), M even in 4..16, aad_len < 0xFF00
// (0: no AAD block and a clear Adata flag), payload_len < 2^(8 L).  aad may be null when aad_len is 0.
inline CcmFormat ccm_format(const uint8_t *nonce, size_t nonce_len, int M, const uint8_t *aad, size_t aad_len,
                            size_t payload_len, CcmFrame &f) {
    f = CcmFrame{};
    if (nonce_len < 7 || nonce_len > 13) return CCM_FMT_NONCE;
    if (M < 4 || M > 16 || (M & 1)) return CCM_FMT_TAG;
    if (aad_len >= kCcmAadLimit) return CCM_FMT_AAD;
    const int L = 15 - (int)nonce_len;
    if (L < 8 && ((uint64_t)payload_len >> (8 * L)) != 0) return CCM_FMT_LEN;
    f.L = L;
    f.M = M;
    f.aad_len = aad_len;
    f.payload_len = payload_len;
    auto be = [&](uint8_t *block, uint64_t v) {  // the last L bytes, big-endian
        for (int i = 0; i < L; i++) block[15 - i] = (uint8_t)(v >> (8 * i));
    };
    const size_t n_blk = payload_len / 16 + (payload_len % 16 != 0);
    f.ctr.assign((n_blk + 1) * 16, 0);
    for (size_t i = 0; i <= n_blk; i++) {
        uint8_t *a = &f.ctr[i * 16];
        a[0] = (uint8_t)(L - 1);
        for (size_t j = 0; j < nonce_len; j++) a[1 + j] = nonce[j];
        be(a, i);
    }
    const size_t aad_bytes = aad_len ? 2 + aad_len : 0;
    const size_t aad_blk = aad_bytes / 16 + (aad_bytes % 16 != 0), n_mac = 1 + aad_blk + n_blk;
    f.mac.assign(n_mac * 16, 0);
    f.src.assign(n_mac * 16, -1);
    uint8_t *b0 = f.mac.data();
    b0[0] = (uint8_t)((aad_len ? 64 : 0) | (8 * ((M - 2) / 2)) | (L - 1));
    for (size_t j = 0; j < nonce_len; j++) b0[1 + j] = nonce[j];
    be(b0, payload_len);
    if (aad_len) {
        uint8_t *a = &f.mac[16];
        a[0] = (uint8_t)(aad_len >> 8);
        a[1] = (uint8_t)aad_len;
        for (size_t j = 0; j < aad_len; j++) a[2 + j] = aad[j];
    }
    for (size_t q = 0; q < payload_len; q++) f.src[(1 + aad_blk) * 16 + q] = (int64_t)q;
    return CCM_FMT_OK;
}

// ---- the plan of a batch of public blocks ----
// One public 16-byte block under key slot `slot`.  The forward cipher writes the first len (0..16) bytes of its
// output at byte out_byte of the concatenated result, as a CtrBlock's.
struct PubBlock {
    int32_t slot;
    uint8_t bytes[16];
    int64_t out_byte;
    int32_t len;
};

// ctr_plan_multi for arbitrary blocks: a group is a distinct (slot, pos, byte value), groups in first-appearance
// order (blocks in order, positions 0..15 within a block).  On iv || be64(counter) blocks it is ctr_plan_multi's plan.
inline void pub_plan(const PubBlock *blocks, size_t n, CtrPlanMulti &plan) {
    plan = CtrPlanMulti{};
    plan.map.assign(n * 16, 0);
    plan.block_slot.resize(n);
    plan.block_out.resize(n);
    plan.block_len.resize(n);
    size_t cap = 64;
    while (cap < n * 32) cap *= 2;
    std::vector<uint64_t> keys(cap, UINT64_MAX);
    std::vector<int32_t> vals(cap, -1);
    for (size_t i = 0; i < n; i++) {
        const PubBlock &b = blocks[i];
        plan.block_slot[i] = b.slot;
        plan.block_out[i] = b.out_byte;
        plan.block_len[i] = b.len;
        for (int pos = 0; pos < 16; pos++) {
            const uint8_t v = b.bytes[pos];
            const uint64_t key = ((uint64_t)(uint32_t)b.slot << 16) | (uint64_t)(pos << 8) | v;
            size_t h = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & (cap - 1);
            while (keys[h] != UINT64_MAX && keys[h] != key) h = (h + 1) & (cap - 1);
            if (keys[h] == UINT64_MAX) {
                keys[h] = key;
                vals[h] = (int32_t)plan.groups.size();
                plan.groups.push_back((uint16_t)((pos << 8) | v));
                plan.group_slot.push_back(b.slot);
            }
            plan.map[i * 16 + pos] = vals[h];
        }
    }
}

// ---- the chain's linear step ----
// How byte `pos` of the MAC block of stream s enters a step: src[s * 16 + pos] >= 0 is the index of the payload
// byte in the result buffer, a negative value -(v + 1) the public byte v.
TAE_LIN_HD int64_t ccm_src_public(uint8_t v) { return -(int64_t)v - 1; }

// Word t of the round-0 state [n][128][L] of a chain step.  x [n][128][L] is the previous cipher output
// Xk = X' + rk_nr, plain [..][8][L] the result buffer of the first pass (P = S' + rk_nr + C), rk a key table
// whose slot key_of[s] (stride key_stride, round r at 128 r L) is the key of stream s.
//   public byte v:   Xk + trivial(v) + rk_0
//   payload byte q:  Xk + P[q] - 2 rk_nr + rk_0  =  X' + S' + C + rk_0: the last round key is removed word for word,
//                    so the sum never holds a key bit twice
// The mode is uniform over the 8 L words of a byte, so the reads stay contiguous runs.
TAE_LIN_HD uint64_t ccm_absorb_word(const uint64_t *x, const uint64_t *plain, const uint64_t *rk, const int64_t *src,
                                    size_t t, int L, const int32_t *key_of, size_t key_stride, int nr) {
    const AesWord w = aes_word(t, L);
    const size_t k = (size_t)(w.pos * 8 + w.bit) * L + w.coef;
    const uint64_t *key = keyed_rk(rk, key_of, key_stride, w.blk);
    const int64_t s = src[w.blk * 16 + w.pos];
    uint64_t v = x[t] + key[k];
    if (s >= 0)
        v += plain[((size_t)s * 8 + w.bit) * L + w.coef] - 2 * key[(size_t)128 * nr * L + k];
    else if (w.coef == (size_t)L - 1)
        v += public_bit((int)(-(s + 1)), w.bit);
    return v;
}

// Word t of the tag differences [n][8 M][L] of the streams in chain order: Xk_last + S_0 - 2 rk_nr + trivial(U),
// x and s0 [n][128][L], tags [n][M] the received (encrypted) tags.  Stream s is written at out_of[s].
TAE_LIN_HD void ccm_tag_word(const uint64_t *x, const uint64_t *s0, const uint64_t *rk, const uint8_t *tags, int M,
                             const int32_t *out_of, uint64_t *out, size_t t, int L, const int32_t *key_of,
                             size_t key_stride, int nr) {
    const size_t coef = t % L, ct = t / L;
    const size_t s = ct / (size_t)(8 * M), i = ct - s * (size_t)(8 * M);  // the stream, and byte * 8 + bit of its tag
    const size_t k = i * L + coef;
    const uint64_t *key = keyed_rk(rk, key_of, key_stride, s);
    uint64_t v = x[s * 128 * (size_t)L + k] + s0[s * 128 * (size_t)L + k] - 2 * key[(size_t)128 * nr * L + k];
    if (coef == (size_t)L - 1) v += public_bit(tags[s * M + (i >> 3)], (int)(i & 7));
    out[((size_t)out_of[s] * 8 * M + i) * L + coef] = v;
}

}  // namespace tae
