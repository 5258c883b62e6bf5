// XTS-AES (IEEE 1619 / NIST SP 800-38E) on the 1-bit model: the tweak mask of block j of a data unit as a leveled
// linear layer, in the style of aes_linear.hpp and aes_inv.hpp.
//
//   T = Enc_K2(tweak)      M_j = alpha^j T      P_j = Dec_K1(C_j ^ M_j) ^ M_j
//
// alpha^j T is the multiplication by x^j in GF(2^128) modulo x^128 + x^7 + x^2 + x + 1.  Coefficient k of the
// polynomial is bit k & 7, counted from the LSB, of byte k >> 3 of the 16-byte value; the project stores bytes
// MSB first, so coefficient k is ciphertext xts_ct_of_coef(k) = 8 (k >> 3) + 7 - (k & 7) of a block.
//
// Over GF(2) the mask is M_j = A_j T, column i of A_j being x^(i + j) mod p.  On ciphertexts, output bit k of the
// mask is the LWE sum (u64 addition) of the tweak ciphertexts i with A_j[k][i] = 1: the row list of k.  The row
// lists of a set of distinct j form a fixed-width table [n_sets][128][width] of source ciphertext indices in the
// project's bit order, padded with -1 up to the set's largest row weight.  The device kernel
// (aes_xts_mask_kernel in aes_engine.hip) is a grid-stride loop around xts_mask_word, so a host program runs the
// same arithmetic (tests/native/aes_xts_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TAE_XTS_HD __host__ __device__ inline
#else
#define TAE_XTS_HD inline
#endif

namespace tae {

// an element of GF(2^128): coefficient k is bit k & 63 of (k < 64 ? lo : hi)
struct Gf128 {
    uint64_t lo, hi;
};

constexpr int xts_ct_of_coef(int k) { return 8 * (k >> 3) + 7 - (k & 7); }

// a * x: the byte-wise left shift with carry of IEEE 1619, 0x87 into byte 0 on carry out of byte 15
constexpr Gf128 xts_alpha(Gf128 a) {
    return {(a.lo << 1) ^ ((a.hi >> 63) ? 0x87u : 0u), (a.hi << 1) | (a.lo >> 63)};
}

constexpr Gf128 xts_gf_mul(Gf128 a, Gf128 b) {
    Gf128 r{0, 0};
    for (int k = 0; k < 128; k++) {
        if (((k < 64 ? b.lo : b.hi) >> (k & 63)) & 1) {
            r.lo ^= a.lo;
            r.hi ^= a.hi;
        }
        a = xts_alpha(a);
    }
    return r;
}

// x^j by square-and-multiply: at most 64 squarings, whatever the block index
constexpr Gf128 xts_x_pow(uint64_t j) {
    Gf128 r{1, 0}, sq{2, 0};
    for (; j; j >>= 1) {
        if (j & 1) r = xts_gf_mul(r, sq);
        sq = xts_gf_mul(sq, sq);
    }
    return r;
}

// A_j by rows, in the project's bit order: rows[o] lists the tweak ciphertexts summed into mask ciphertext o,
// ascending.  Column i is x^(i + j), stepped from x^j.
inline void xts_rows_of(uint64_t j, std::vector<int16_t> rows[128]) {
    std::vector<int16_t> by_coef[128];
    Gf128 col = xts_x_pow(j);
    for (int i = 0; i < 128; i++, col = xts_alpha(col))
        for (int k = 0; k < 128; k++)
            if (((k < 64 ? col.lo : col.hi) >> (k & 63)) & 1) by_coef[k].push_back((int16_t)xts_ct_of_coef(i));
    for (int k = 0; k < 128; k++) {
        std::vector<int16_t> &r = rows[xts_ct_of_coef(k)];
        r = by_coef[k];
        for (size_t a = 1; a < r.size(); a++)  // ascending ciphertext order: insertion sort of a short list
            for (size_t b = a; b > 0 && r[b - 1] > r[b]; b--) {
                const int16_t t = r[b];
                r[b] = r[b - 1];
                r[b - 1] = t;
            }
    }
}

// w(j): the largest row weight of A_j, which sets the noise of block j's mask
inline int xts_row_weight(uint64_t j) {
    std::vector<int16_t> rows[128];
    xts_rows_of(j, rows);
    size_t w = 0;
    for (const auto &r : rows) w = r.size() > w ? r.size() : w;
    return (int)w;
}

// The row lists of the distinct block indices of a call and, per block, its data unit and its row-list set
struct XtsPlan {
    int width = 0;               // the largest row weight of the sets
    std::vector<int16_t> rows;   // [n_sets][128][width], -1 padded
    std::vector<int32_t> unit_of, set_of;  // [nb]
    size_t n_sets() const { return width ? rows.size() / (128 * (size_t)width) : 0; }
};

// block b of the call is block block_index[b] of data unit unit_of[b] (unit_of == nullptr: unit 0)
inline void xts_plan(const int32_t *unit_of, const uint64_t *block_index, size_t nb, XtsPlan &plan) {
    std::map<uint64_t, int32_t> sets;
    std::vector<std::vector<int16_t>> lists;  // [set * 128 + o]
    plan.unit_of.resize(nb);
    plan.set_of.resize(nb);
    plan.width = 0;
    for (size_t b = 0; b < nb; b++) {
        plan.unit_of[b] = unit_of ? unit_of[b] : 0;
        auto it = sets.find(block_index[b]);
        if (it == sets.end()) {
            it = sets.emplace(block_index[b], (int32_t)sets.size()).first;
            std::vector<int16_t> rows[128];
            xts_rows_of(block_index[b], rows);
            for (auto &r : rows) {
                plan.width = (int)r.size() > plan.width ? (int)r.size() : plan.width;
                lists.push_back(std::move(r));
            }
        }
        plan.set_of[b] = it->second;
    }
    plan.rows.assign(lists.size() * (size_t)plan.width, -1);
    for (size_t r = 0; r < lists.size(); r++)
        for (size_t q = 0; q < lists[r].size(); q++) plan.rows[r * plan.width + q] = lists[r][q];
}

// Word t of the masks [nb][128][L]: coefficient t % L of ciphertext o = (t / L) & 127 of block (t / L) >> 7, the
// sum of that coefficient of the tweak ciphertexts in row o of the block's set.  tweaks [n_units][128][L].  The
// unit and the set are uniform over the L coefficients of a ciphertext, so every read is a contiguous run.
TAE_XTS_HD uint64_t xts_mask_word(const uint64_t *tweaks, const int16_t *rows, int width, const int32_t *unit_of,
                                  const int32_t *set_of, size_t t, int L) {
    const size_t coef = t % L, ct = t / L, blk = ct >> 7;
    const int16_t *row = rows + ((size_t)set_of[blk] * 128 + (ct & 127)) * width;
    const uint64_t *T = tweaks + (size_t)unit_of[blk] * 128 * L + coef;
    uint64_t acc = 0;
    for (int q = 0; q < width; q++) {
        const int src = row[q];
        if (src < 0) break;
        acc += T[(size_t)src * L];
    }
    return acc;
}

}  // namespace tae
