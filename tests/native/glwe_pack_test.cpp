// Host check of the packed-I/O index maps (csrc/glwe_pack.hpp) for N = 8 and N = 512, k = 1 and 4:
//   - extracting coefficient j of a random GLWE and taking the LWE phase under the flattened key gives
//     coefficient j of the GLWE phase (schoolbook negacyclic products), for every j;
//   - j = 0 is the rule of the blind rotation's sample extraction (a[pN] = A_p[0], a[pN + i] = -A_p[N - i]);
//   - rotate-and-sum of count in {1, N - 1, N} polynomials equals the sum of exact negacyclic products with the
//     monomials X^j;
//   - the 32-bit wire form rounds to the nearest multiple of 2^32.
// Stand-alone: built plain and with -fsanitize=address,undefined by tests/test_glwe_pack.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/glwe_pack.hpp"

namespace gp = tae::glwe_pack;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// c = a * b mod X^N + 1, mod 2^64
static std::vector<uint64_t> negacyclic_mul(const uint64_t *a, const uint64_t *b, int N) {
    std::vector<uint64_t> c(N, 0);
    for (int j = 0; j < N; j++) {
        if (!b[j]) continue;  // binary keys and monomials are sparse
        for (int i = 0; i < N; i++) {
            const uint64_t t = a[i] * b[j];
            if (i + j < N)
                c[i + j] += t;
            else
                c[i + j - N] -= t;
        }
    }
    return c;
}

static int failures = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            if (failures++ < 10) {           \
                std::printf("FAIL: ");       \
                std::printf(__VA_ARGS__);    \
                std::printf("\n");           \
            }                                \
        }                                    \
    } while (0)

static void check_extract(int N, int k) {
    const size_t glwe = (size_t)(k + 1) * N;
    std::vector<uint64_t> ct(glwe), key((size_t)k * N), phase(N), lwe((size_t)k * N + 1);
    for (auto &w : ct) w = rnd();
    for (auto &s : key) s = rnd() & 1;
    for (int c = 0; c < N; c++) phase[c] = ct[(size_t)k * N + c];
    for (int p = 0; p < k; p++) {
        const auto prod = negacyclic_mul(&ct[(size_t)p * N], &key[(size_t)p * N], N);
        for (int c = 0; c < N; c++) phase[c] -= prod[c];
    }
    for (int j = 0; j < N; j++) {
        gp::extract_lwe(ct.data(), k, N, j, lwe.data());
        uint64_t ph = lwe[(size_t)k * N];
        for (size_t i = 0; i < (size_t)k * N; i++) ph -= lwe[i] * key[i];
        CHECK(ph == phase[j], "extract N=%d k=%d j=%d: LWE phase differs from the GLWE phase", N, k, j);
    }
    gp::extract_lwe(ct.data(), k, N, 0, lwe.data());
    for (int t = 0; t < k * N; t++) {
        const int p = t / N, j = t - p * N;
        const uint64_t want = j == 0 ? ct[(size_t)p * N] : (0 - ct[(size_t)p * N + N - j]);
        CHECK(lwe[t] == want, "extract N=%d k=%d: j = 0 differs from the existing rule at word %d", N, k, t);
    }
    CHECK(lwe[(size_t)k * N] == ct[(size_t)k * N], "extract N=%d k=%d: body of j = 0", N, k);
}

static void check_rotate_sum(int N, int k, int count) {
    const size_t glwe = (size_t)(k + 1) * N;
    std::vector<uint64_t> in((size_t)count * glwe), out(glwe), want(glwe, 0), mono(N);
    for (auto &w : in) w = rnd();
    gp::rotate_sum(in.data(), count, k, N, out.data());
    for (int j = 0; j < count; j++) {
        for (int c = 0; c < N; c++) mono[c] = c == j;
        for (int p = 0; p <= k; p++) {
            const auto prod = negacyclic_mul(&in[(size_t)j * glwe + (size_t)p * N], mono.data(), N);
            for (int c = 0; c < N; c++) want[(size_t)p * N + c] += prod[c];
        }
    }
    for (size_t t = 0; t < glwe; t++)
        CHECK(out[t] == want[t], "rotate_sum N=%d k=%d count=%d: word %zu", N, k, count, t);
}

int main() {
    for (int N : {8, 512})
        for (int k : {1, 4}) {
            check_extract(N, k);
            for (int count : {1, N - 1, N}) check_rotate_sum(N, k, count);
        }
    CHECK(gp::glwe_count(1, 512) == 1 && gp::glwe_count(512, 512) == 1 && gp::glwe_count(513, 512) == 2 &&
              gp::glwe_count(1030, 512) == 3,
          "glwe_count");
    const uint64_t words[] = {0, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFF7FFFFFFFull, 0xFFFFFFFF80000000ull, 1ull << 63};
    for (uint64_t w : words) {
        const uint64_t back = gp::widen_word(gp::narrow_word(w));
        const uint64_t err = back - w, mag = (int64_t)err < 0 ? 0 - err : err;
        CHECK(mag <= (1ull << 31), "narrow / widen of %016llx is off by more than 2^31", (unsigned long long)w);
    }
    CHECK(gp::narrow_word(0xFFFFFFFF80000000ull) == 0, "narrowing wraps at the top");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
