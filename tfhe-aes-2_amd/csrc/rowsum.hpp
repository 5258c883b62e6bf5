// LWE row sums: output ciphertext r = the u64 sum of listed source ciphertexts (+ a public bit).  The one linear
// layer XTS's tweak masks (aes_xts.hpp) and GCM's squares, products and tag rows (aes_gcm.hpp) share (DESIGN.md
// 5.15).  Host/device in the style of aes_linear.hpp: the device kernel (rowsum_kernel in aes_engine.hip) is a
// grid-stride loop around rowsum_word, so a host program runs the same arithmetic (tests/native/rowsum_test.cpp);
// rowsum2_word / rowsum2_kernel are the same over two source arrays (tests/native/rowsum2_test.cpp).
//
// The lists are CSR: list l is src[row_start[l] .. row_start[l + 1]) into one source array [n_src][L]; their widths
// range from 0 to 64, so no table padded to the largest.  Nullable per-output-row arrays, as aes_linear.hpp's:
//   list_of[r]  the list that output row r sums            (null: list r)
//   base_of[r]  added to every source index of that row    (null: 0)
//   pub_bit[r]  0 / 1, added as a trivial encryption       (null: none)
// so "the same lists under another base" (block j of another data unit, the same product of another pair) costs two
// integers per row, not a copy of the lists.  u64 addition wraps and commutes: any order gives the same words.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TAE_ROWSUM_HD __host__ __device__ inline
#else
#define TAE_ROWSUM_HD inline
#endif

namespace tae {

struct RowPlan {
    std::vector<int32_t> row_start{0};
    std::vector<int32_t> src;
    std::vector<int32_t> list_of, base_of;  // empty (null), or one per output row
    std::vector<uint8_t> pub_bit;           // empty (null), or one 0 / 1 per output row
    size_t n_lists() const { return row_start.size() - 1; }
    size_t n_rows() const { return list_of.empty() ? n_lists() : list_of.size(); }
    void end_row() { row_start.push_back((int32_t)src.size()); }
    int width(size_t l) const { return row_start[l + 1] - row_start[l]; }
    int max_width() const {
        int w = 0;
        for (size_t l = 0; l < n_lists(); l++) w = width(l) > w ? width(l) : w;
        return w;
    }
};

template <class T>
const T *rowplan_ptr(const std::vector<T> &v) {
    return v.empty() ? nullptr : v.data();
}

// what a launch relies on: whole lists, list_of within the lists, base + src within the n_src sources for every row,
// one public bit per row or none
inline bool rowplan_ok(const RowPlan &p, size_t n_src) {
    if (p.row_start.empty() || p.row_start[0] != 0 || (size_t)p.row_start.back() != p.src.size()) return false;
    for (size_t l = 0; l < p.n_lists(); l++)  // before any list is walked: increasing from 0 to src.size() bounds all
        if (p.row_start[l + 1] < p.row_start[l]) return false;
    std::vector<int32_t> top(p.n_lists(), -1);  // the largest index of every list
    for (size_t l = 0; l < p.n_lists(); l++) {
        for (int32_t q = p.row_start[l]; q < p.row_start[l + 1]; q++) {
            if (p.src[q] < 0) return false;
            top[l] = p.src[q] > top[l] ? p.src[q] : top[l];
        }
    }
    const size_t n_rows = p.n_rows();
    if (!p.base_of.empty() && p.base_of.size() != n_rows) return false;
    if (!p.pub_bit.empty() && p.pub_bit.size() != n_rows) return false;
    for (size_t r = 0; r < n_rows; r++) {
        const int32_t l = p.list_of.empty() ? (int32_t)r : p.list_of[r], base = p.base_of.empty() ? 0 : p.base_of[r];
        if (l < 0 || (size_t)l >= p.n_lists() || base < 0) return false;
        if (top[(size_t)l] >= 0 && (size_t)base + (size_t)top[(size_t)l] >= n_src) return false;
    }
    for (uint8_t b : p.pub_bit)
        if (b > 1) return false;
    return true;
}

// Word t of the row sums [n_rows][L]: coefficient t % L of row t / L, plus pub_bit << 63 in the body word.  The list
// and the base are uniform over the L words of a row, so every read is a contiguous run of L words over its lanes.
TAE_ROWSUM_HD uint64_t rowsum_word(const uint64_t *sources, const int32_t *row_start, const int32_t *src,
                                   const int32_t *list_of, const int32_t *base_of, const uint8_t *pub_bit, size_t t,
                                   int L) {
    const size_t coef = t % L, row = t / L, list = list_of ? (size_t)list_of[row] : row;
    const uint64_t *S = sources + (base_of ? (size_t)base_of[row] * L : 0) + coef;
    uint64_t acc = 0;
    for (int32_t q = row_start[list]; q < row_start[list + 1]; q++) acc += S[(size_t)src[q] * L];
    if (pub_bit && coef == (size_t)L - 1) acc += (uint64_t)pub_bit[row] << 63;
    return acc;
}

// the same word from a plan's own arrays
inline uint64_t rowsum_word(const uint64_t *sources, const RowPlan &p, size_t t, int L) {
    return rowsum_word(sources, p.row_start.data(), rowplan_ptr(p.src), rowplan_ptr(p.list_of), rowplan_ptr(p.base_of),
                       rowplan_ptr(p.pub_bit), t, L);
}

// ---- two source arrays: A [n_a][L] and B [n_b][L] read as one array of n_a + n_b sources without
// being one allocation.  The effective index base_of[row] + src[q] reads A below n_a and B at index - n_a from there
// on.  GCM over key tables sums bits of a caller's power tables (A, read in place) and bits of the call's kept E(J0)
// blocks (B): no table block is staged next to them. ----
inline bool rowplan2_ok(const RowPlan &p, size_t n_a, size_t n_b) { return rowplan_ok(p, n_a + n_b); }

// Word t of the row sums over the two arrays.  Which array a source lies in depends on the row and the list entry
// alone, so the choice is uniform over the L words of a row and every read is a contiguous run of L words.
TAE_ROWSUM_HD uint64_t rowsum2_word(const uint64_t *A, size_t n_a, const uint64_t *B, const int32_t *row_start,
                                    const int32_t *src, const int32_t *list_of, const int32_t *base_of,
                                    const uint8_t *pub_bit, size_t t, int L) {
    const size_t coef = t % L, row = t / L, list = list_of ? (size_t)list_of[row] : row;
    const size_t base = base_of ? (size_t)base_of[row] : 0;
    uint64_t acc = 0;
    for (int32_t q = row_start[list]; q < row_start[list + 1]; q++) {
        const size_t s = base + (size_t)src[q];
        acc += s < n_a ? A[s * L + coef] : B[(s - n_a) * L + coef];
    }
    if (pub_bit && coef == (size_t)L - 1) acc += (uint64_t)pub_bit[row] << 63;
    return acc;
}

inline uint64_t rowsum2_word(const uint64_t *A, size_t n_a, const uint64_t *B, const RowPlan &p, size_t t, int L) {
    return rowsum2_word(A, n_a, B, p.row_start.data(), rowplan_ptr(p.src), rowplan_ptr(p.list_of),
                        rowplan_ptr(p.base_of), rowplan_ptr(p.pub_bit), t, L);
}

}  // namespace tae
