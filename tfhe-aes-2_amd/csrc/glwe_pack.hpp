// Packed ciphertext I/O: index maps between GLWE-packed bits and big-key LWEs, shared by the
// host (client.cpp, tests/native/glwe_pack_test.cpp) and the device kernels (kernels.hip).
//
// Format: `count` bits occupy G = ceil(count / N) GLWEs [G][(k+1)N], mask polynomials first, body last.  Bit j
// sits at coefficient j % N of GLWE j / N, encoded bit << 63.
//
// Sample extraction of coefficient j of a GLWE (A_0 .. A_{k-1}, B) into an LWE under the flattened GLWE key
// (exact, no noise added):
//   a[pN + i] = A_p[j - i]        for i <= j
//   a[pN + i] = -A_p[N + j - i]   for i > j
//   b         = B[j]
// (coefficient j of A_p S_p mod X^N + 1 is sum_i S_p[i] a[pN + i]).  j = 0 is the blind rotation's
// sample_extract_store.
//
// Multiplication of a polynomial P by the monomial X^j, 0 <= j < N (negacyclic):
//   (X^j P)[c] = P[c - j]         for c >= j
//   (X^j P)[c] = -P[N + c - j]    for c < j
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TAE_PACK_HD __host__ __device__
#else
#define TAE_PACK_HD
#endif

namespace tae {
namespace glwe_pack {

// bits per packing chunk on the device: whole GLWEs, at most 16384 bits of [glwe] keyswitch scratch (335 MB)
constexpr size_t kChunkBits = 16384;

TAE_PACK_HD inline size_t glwe_count(size_t count, int N) { return (count + (size_t)N - 1) / (size_t)N; }

// Mask word i (0 <= i < N) of polynomial p in the extraction of coefficient j: poly[src] or its negation.
TAE_PACK_HD inline int extract_src(int N, int j, int i, bool &negate) {
    negate = i > j;
    return negate ? N + j - i : j - i;
}

TAE_PACK_HD inline uint64_t extract_word(const uint64_t *poly, int N, int j, int i) {
    bool neg;
    const uint64_t v = poly[extract_src(N, j, i, neg)];
    return neg ? 0 - v : v;
}

// Coefficient c of X^j P: P[src] or its negation.
TAE_PACK_HD inline int rotate_src(int N, int j, int c, bool &negate) {
    negate = c < j;
    return negate ? N + c - j : c - j;
}

TAE_PACK_HD inline uint64_t rotate_word(const uint64_t *poly, int N, int j, int c) {
    bool neg;
    const uint64_t v = poly[rotate_src(N, j, c, neg)];
    return neg ? 0 - v : v;
}

// Host forms over whole ciphertexts.
// GLWE [(k+1)N] -> LWE [kN + 1] of coefficient j
inline void extract_lwe(const uint64_t *glwe, int k, int N, int j, uint64_t *lwe) {
    for (int p = 0; p < k; p++)
        for (int i = 0; i < N; i++) lwe[(size_t)p * N + i] = extract_word(glwe + (size_t)p * N, N, j, i);
    lwe[(size_t)k * N] = glwe[(size_t)k * N + j];
}

// out [(k+1)N] = sum_{j < count} X^j in_j, in [count][(k+1)N], count <= N
inline void rotate_sum(const uint64_t *in, int count, int k, int N, uint64_t *out) {
    const size_t glwe = (size_t)(k + 1) * N;
    for (int p = 0; p <= k; p++)
        for (int c = 0; c < N; c++) {
            uint64_t acc = 0;
            for (int j = 0; j < count; j++) acc += rotate_word(in + (size_t)j * glwe + (size_t)p * N, N, j, c);
            out[(size_t)p * N + c] = acc;
        }
}

// The 32-bit wire form of a packed word (round to the top 32 bits) and back.
TAE_PACK_HD inline uint32_t narrow_word(uint64_t w) { return (uint32_t)((w + (1ull << 31)) >> 32); }
TAE_PACK_HD inline uint64_t widen_word(uint32_t w) { return (uint64_t)w << 32; }

}  // namespace glwe_pack
}  // namespace tae
