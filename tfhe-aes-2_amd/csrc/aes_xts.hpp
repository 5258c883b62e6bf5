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
// mask is the LWE sum (u64 addition) of the tweak ciphertexts i with A_j[k][i] = 1: the row list of k, in the
// project's bit order.  xts_plan turns the blocks of a call into a RowPlan (rowsum.hpp): the 128 lists of every
// distinct block index once, and per mask ciphertext its list and the first tweak ciphertext of its data unit, so the
// shared row-sum kernel computes the masks and a host program the same words (tests/native/aes_xts_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include "rowsum.hpp"

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

// The masks [nb][128] of a call as row sums over the tweak ciphertexts [n_units][128]: block b of the call is block
// block_index[b] of data unit unit_of[b] (unit_of == nullptr: unit 0).  The lists of the distinct block indices
// once, set s at lists 128 s ..; mask ciphertext o of block b sums list 128 set(b) + o at base 128 unit_of[b]
inline RowPlan xts_plan(const int32_t *unit_of, const uint64_t *block_index, size_t nb) {
    RowPlan plan;
    std::map<uint64_t, int32_t> sets;
    plan.list_of.reserve(nb * 128);
    plan.base_of.reserve(nb * 128);
    for (size_t b = 0; b < nb; b++) {
        auto it = sets.find(block_index[b]);
        if (it == sets.end()) {
            it = sets.emplace(block_index[b], (int32_t)sets.size()).first;
            std::vector<int16_t> rows[128];
            xts_rows_of(block_index[b], rows);
            for (const auto &r : rows) {
                plan.src.insert(plan.src.end(), r.begin(), r.end());
                plan.end_row();
            }
        }
        for (int32_t o = 0; o < 128; o++) {
            plan.list_of.push_back(it->second * 128 + o);
            plan.base_of.push_back((unit_of ? unit_of[b] : 0) * 128);
        }
    }
    return plan;
}

}  // namespace tae
