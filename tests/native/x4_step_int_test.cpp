// Host-side check of the lane-level integer helpers of br512x4's CMux step (fft_device.hpp):
//   torus_add_fast2_sh<8>  against acc + from_torus_bits(x 2^-8) and the oracle's or_from_torus, with its
//                          documented refusals (`ok` false exactly when s is outside [12, 63] or the high
//                          dword of the magnitude is 0x80000000), next to its predecessor torus_add_fast_sh<8>;
//   decompose16p_fast      against decompose16p and the oracle's or_decompose, with its documented refusals
//                          (`ok` false exactly when a biased field is zero);
//   rot_diff<9> / <10>     against a naive negacyclic ACC X^e - ACC for every e and j, and the digits the
//                          kernel takes from its outputs against the oracle's or_decompose of the naive ones.
// Built and run by tests/test_x4_step_int.py (CPU only).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/fft_device.hpp"

extern "C" {
uint64_t or_from_torus(double x);
void or_decompose(uint64_t x, int base_log, int levels, int64_t *digits);
}

static int fails = 0;
static long n_ok = 0, n_refused = 0, n_refused_hi = 0;

// the documented refusal rule, restated from the bits of y alone
static bool documented_ok(double y, bool &hi_case) {
    uint64_t b;
    std::memcpy(&b, &y, 8);
    const int s = (int)((b >> 52) & 0x7ff) - 1011 - 8;
    hi_case = false;
    if (s < 12 || s > 63) return false;
    const uint64_t m = (b & 0xFFFFFFFFFFFFFull) | (1ull << 52);
    hi_case = (uint32_t)((m << s) >> 32) == 0x80000000u;
    return !hi_case;
}

static void check_tail(double y) {
    const double x = y * 0x1p-8;  // exact: no input here is subnormal after the scaling
    const uint64_t want = or_from_torus(x);
    if (tae::from_torus_bits(x) != want && fails++ < 10) printf("from_torus_bits(%a) differs from the oracle\n", x);
    uint64_t yb;
    std::memcpy(&yb, &y, 8);
    const uint64_t acc0 = 0x0123456789abcdefull ^ (yb * 0x9E3779B97F4A7C15ull);
    bool ok, ok_old, hi_case;
    const uint64_t got = tae::torus_add_fast2_sh<8>(y, acc0, ok);
    const uint64_t old = tae::torus_add_fast_sh<8>(y, acc0, ok_old);
    const bool doc = documented_ok(y, hi_case);
    if (ok != doc && fails++ < 10) printf("torus_add_fast2_sh<8>(%a): ok %d, documented %d\n", y, (int)ok, (int)doc);
    if (ok && got != acc0 + want && fails++ < 10)
        printf("torus_add_fast2_sh<8>(%a): got %016llx want %016llx\n", y, (unsigned long long)(got - acc0),
               (unsigned long long)want);
    if (ok_old && old != acc0 + want && fails++ < 10)
        printf("torus_add_fast_sh<8>(%a): got %016llx want %016llx\n", y, (unsigned long long)(old - acc0),
               (unsigned long long)want);
    if (ok && !ok_old && fails++ < 10) printf("torus_add_fast2_sh<8>(%a) accepts what its predecessor refuses\n", y);
    ok ? n_ok++ : n_refused++;
    n_refused_hi += hi_case;
}

// y with y 2^-8 2^64 = m 2^s for a 53-bit significand m (bit 52 set)
static double from_ms(uint64_t m, int s, bool neg) {
    const double y = std::ldexp((double)m, s - 64 + 8);
    return neg ? -y : y;
}

// decompose16p_fast: `ok` false exactly when a biased field of x0 or x1 is zero, and the oracle's digits otherwise
static long n_dec_ok = 0, n_dec_refused = 0;
template <int LEV, int B>
static void check_fast(uint64_t x0, uint64_t x1) {
    constexpr int nrb = 64 - B * LEV;
    uint64_t bias = 1ull << (nrb - 1);
    for (int i = 0; i < LEV; i++) bias += 1ull << (nrb + B * i + B - 1);
    bool doc = true;
    for (int i = 0; i < LEV; i++)
        for (uint64_t x : {x0, x1}) doc &= (((x + bias) >> (nrb + B * i)) & ((1ull << B) - 1)) != 0;
    uint32_t d[LEV], ref[LEV];
    int64_t r0[LEV], r1[LEV];
    bool ok;
    tae::decompose16p_fast<LEV, B>(x0, x1, d, ok);
    tae::decompose16p<LEV, B>(x0, x1, ref);
    or_decompose(x0, B, LEV, r0);
    or_decompose(x1, B, LEV, r1);
    if (ok != doc && fails++ < 10)
        printf("decompose16p_fast<%d,%d>(%016llx, %016llx): ok %d, documented %d\n", LEV, B, (unsigned long long)x0,
               (unsigned long long)x1, (int)ok, (int)doc);
    for (int l = 0; l < LEV; l++) {
        if (((int16_t)(ref[l] & 0xFFFF) != r0[l] || (int16_t)(ref[l] >> 16) != r1[l]) && fails++ < 10)
            printf("decompose16p<%d,%d>(%016llx, %016llx) level %d differs from the oracle\n", LEV, B,
                   (unsigned long long)x0, (unsigned long long)x1, l + 1);
        if (ok && d[l] != ref[l] && fails++ < 10)
            printf("decompose16p_fast<%d,%d>(%016llx, %016llx) level %d: got %08x want %08x\n", LEV, B,
                   (unsigned long long)x0, (unsigned long long)x1, l + 1, d[l], ref[l]);
    }
    ok ? n_dec_ok++ : n_dec_refused++;
}

template <int LEV, int B>
static void check_fast_all(std::mt19937_64 &rng, long n) {
    constexpr int nrb = 64 - B * LEV;
    const uint64_t edges[] = {0, 1, ~0ull, 1ull << 63, (1ull << 63) - 1, 1ull << (nrb - 1), (1ull << (nrb - 1)) - 1,
                              (1ull << nrb) - 1, ~0ull << nrb, (~0ull << nrb) - 1, 0x8008008000000000ull,
                              0x7FF7FF8000000000ull, 0x0800800800000000ull, 0xF7FF7FF7F8000000ull};
    for (uint64_t x : edges)
        for (uint64_t y : edges) check_fast<LEV, B>(x, y);
    for (long i = 0; i < n; i++) {
        uint64_t x = rng(), y = rng();
        if (i & 1) {  // fields on and beside the tie (half a base), with and without the rounding carry below
            const int f = (int)(rng() % LEV);
            const uint64_t fm = ((1ull << B) - 1) << (nrb + B * f);
            x = (x & ~fm) | ((1ull << (B - 1)) - (rng() % 3 == 0)) << (nrb + B * f);
            if (i & 2) x |= (1ull << (nrb + B * f)) - 1;  // all ones below: the carries ripple into the field
            if (i & 4) x &= ~((1ull << (nrb + B * f)) - 1);
        }
        if ((i & 24) == 8) y = x ^ (rng() & ((1ull << nrb) - 1));
        check_fast<LEV, B>(x, y);
    }
}

template <int LOGN>
static void naive_rot_diff(const std::vector<uint64_t> &p, int e, std::vector<uint64_t> &d) {
    constexpr int N = 1 << LOGN;
    for (int i = 0; i < N; i++) {
        const int pos = (i + e) & (2 * N - 1);
        if (pos < N) d[pos] = p[i];
        else d[pos - N] = 0 - p[i];
    }
    for (int i = 0; i < N; i++) d[i] -= p[i];
}

template <int LOGN, bool DIGITS>
static void check_rot(const std::vector<uint64_t> &p) {
    constexpr int N = 1 << LOGN, M = N / 2;
    std::vector<uint64_t> d(N);
    for (int e = 0; e < 2 * N; e++) {
        naive_rot_diff<LOGN>(p, e, d);
        for (int j = 0; j < M; j++) {
            uint64_t x0, x1;
            tae::rot_diff<LOGN>(p.data(), j, e, p[j], p[j + M], x0, x1);
            if ((x0 != d[j] || x1 != d[j + M]) && fails++ < 10)
                printf("rot_diff<%d>(j=%d, e=%d): got %016llx %016llx want %016llx %016llx\n", LOGN, j, e,
                       (unsigned long long)x0, (unsigned long long)x1, (unsigned long long)d[j],
                       (unsigned long long)d[j + M]);
            if (DIGITS) {
                uint32_t dp[3];
                int64_t r0[3], r1[3];
                bool dok;  // as the kernel: the fast digits, decompose16p when they are refused
                tae::decompose16p_fast<3, 12>(x0, x1, dp, dok);
                if (!dok) tae::decompose16p<3, 12>(x0, x1, dp);
                or_decompose(d[j], 12, 3, r0);
                or_decompose(d[j + M], 12, 3, r1);
                for (int l = 0; l < 3; l++)
                    if (((int16_t)(dp[l] & 0xFFFF) != r0[l] || (int16_t)(dp[l] >> 16) != r1[l]) && fails++ < 10)
                        printf("digits(j=%d, e=%d) level %d: got %d %d want %lld %lld\n", j, e, l + 1,
                               (int)(int16_t)(dp[l] & 0xFFFF), (int)(int16_t)(dp[l] >> 16), (long long)r0[l],
                               (long long)r1[l]);
            }
        }
    }
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? atol(argv[1]) : 1000000;
    std::mt19937_64 rng(20240607);
    // ---- torus tail ----
    const double zeros[] = {0.0, -0.0};
    for (double z : zeros) check_tail(z);
    // random doubles across the exponent range: s from -40 to 90, and arbitrary finite bit patterns
    for (long i = 0; i < n; i++) {
        const uint64_t r = rng();
        const uint64_t m = (rng() & 0xFFFFFFFFFFFFFull) | (1ull << 52);
        check_tail(from_ms(m, (int)(r % 131) - 40, (r >> 40) & 1));
        if ((i & 3) == 0) {
            uint64_t b = rng();
            const uint32_t ex = (uint32_t)(b >> 52) & 0x7ff;
            if (ex == 0x7ff || ex < 16) b ^= 1ull << 61;  // finite, and normal after the 2^-8
            double y;
            std::memcpy(&y, &b, 8);
            check_tail(y);
        }
    }
    // the edges of the accepted range and of the predecessor's
    for (int s : {-1, 0, 11, 12, 13, 62, 63, 64, 65})
        for (int k = 0; k < 2000; k++) {
            uint64_t m = (rng() & 0xFFFFFFFFFFFFFull) | (1ull << 52);
            if (k == 0) m = 1ull << 52;
            if (k == 1) m = (1ull << 53) - 1;
            check_tail(from_ms(m, s, false));
            check_tail(from_ms(m, s, true));
        }
    // +-(n + 1/2) 2^8: the i64 saturation (negative) and its refused mirror image
    for (int k = 0; k < 20000; k++) {
        const double h = (double)(int64_t)(k < 1000 ? k : rng() % (1ull << (1 + rng() % 50))) + 0.5;
        check_tail(h * 0x1p8);
        check_tail(-h * 0x1p8);
    }
    // significands whose magnitude has the high dword 0x80000000, low dword zero and non-zero: bit 63 - s set,
    // bits [32 - s, 63 - s) clear, the bits above (shifted out) and below (the low dword, s < 32) free
    for (int s = 12; s <= 63; s++)
        for (int k = 0; k < 200; k++) {
            uint64_t m = (1ull << 52) | (1ull << (63 - s));
            if (64 - s < 52) m |= (rng() << (64 - s)) & 0xFFFFFFFFFFFFFull;
            uint64_t low = 0;
            if (s < 32 && (k & 1)) low = (rng() & ((1ull << (32 - s)) - 1)) | 1;
            m |= low;
            bool hc;
            const double y = from_ms(m, s, false);
            if ((documented_ok(y, hc) || !hc) && fails++ < 10) printf("test bug: m %013llx s %d is no high-dword case\n", (unsigned long long)m, s);
            check_tail(y);
            check_tail(-y);
            // one bit beside it: accepted again
            check_tail(from_ms(m ^ (1ull << (63 - s)), s, k & 2));
            if (s < 63) check_tail(from_ms(m | (1ull << (62 - s)), s, k & 2));
        }
    // ---- fast decomposition: the kernels' shapes ----
    check_fast_all<3, 12>(rng, n);
    check_fast_all<7, 6>(rng, n / 4);
    check_fast_all<1, 13>(rng, n / 4);
    check_fast_all<6, 7>(rng, n / 4);
    check_fast_all<2, 15>(rng, n / 4);
    // ---- rotated difference and its digits ----
    for (int trial = 0; trial < 3; trial++) {
        std::vector<uint64_t> p(512);
        for (auto &v : p) v = rng();
        if (trial == 2)  // rounding ties and extremes of the decomposition
            for (int i = 0; i < 512; i += 3) p[i] = (i & 1) ? ~0ull << (i % 40) : (1ull << 27) * (rng() % 5) + (rng() << 40);
        check_rot<9, true>(p);
    }
    {
        std::vector<uint64_t> p(1024);
        for (auto &v : p) v = rng();
        check_rot<10, false>(p);
    }
    printf("tail: %ld accepted, %ld refused (%ld by the high dword)\n", n_ok, n_refused, n_refused_hi);
    printf("fast decomposition: %ld accepted, %ld refused\n", n_dec_ok, n_dec_refused);
    printf("%s (%d mismatches)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
