// Host check of the two-source row sums (csrc/rowsum.hpp), the arithmetic of rowsum2_kernel on plain
// words: rowsum2_word against a direct double loop at L = 3 and L = 2049, with A and B in separate allocations so that
// an index on the wrong side of the split reads out of bounds under the sanitizer; what rowplan2_ok refuses; and the
// plan a GCM call over key tables builds (gcm_multi_plan_add) for three frames under two slots, replayed on plain bits
// against the single-key plans on each slot's table and against GHASH itself.  Stand-alone: built plain and with
// -fsanitize=address,undefined by tests/test_rowsum2.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/aes_gcm.hpp"
#include "../../tfhe-aes-2_amd/csrc/rowsum.hpp"

using namespace tae;

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                \
        }                                                           \
    } while (0)

static uint64_t next(uint64_t &seed) {
    seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
    return seed ^ (seed >> 29);
}

// every word through rowsum2_word; A / B are exactly n_a L and n_b L words long
static std::vector<uint64_t> run2(const std::vector<uint64_t> &A, const std::vector<uint64_t> &B, const RowPlan &p, int L) {
    const size_t n_a = A.size() / L, n_b = B.size() / L;
    CHECK(rowplan2_ok(p, n_a, n_b));
    std::vector<uint64_t> out(p.n_rows() * L);
    for (size_t t = 0; t < out.size(); t++) out[t] = rowsum2_word(A.data(), n_a, B.data(), p, t, L);
    return out;
}

// the definition, row by row and source by source
static std::vector<uint64_t> direct2(const std::vector<uint64_t> &A, const std::vector<uint64_t> &B, const RowPlan &p,
                                     int L) {
    const size_t n_a = A.size() / L;
    std::vector<uint64_t> out(p.n_rows() * L, 0);
    for (size_t r = 0; r < p.n_rows(); r++) {
        const size_t l = p.list_of.empty() ? r : (size_t)p.list_of[r], base = p.base_of.empty() ? 0 : (size_t)p.base_of[r];
        for (int32_t q = p.row_start[l]; q < p.row_start[l + 1]; q++) {
            const size_t s = base + (size_t)p.src[q];
            for (int c = 0; c < L; c++) out[r * L + c] += s < n_a ? A.at(s * L + c) : B.at((s - n_a) * L + c);
        }
        if (!p.pub_bit.empty()) out[r * L + L - 1] += (uint64_t)p.pub_bit[r] << 63;
    }
    return out;
}

static void word_cases(int L, uint64_t &seed) {
    const size_t n_a = 6, n_b = 5;
    std::vector<uint64_t> A(n_a * L), B(n_b * L);
    for (auto &w : A) w = next(seed);  // full words: the sums wrap
    for (auto &w : B) w = next(seed);
    // lists: across the split (n_a - 1 and n_a together), B alone, A alone, empty, a list below the split that a base
    // carries across it, a wide one over both
    RowPlan lists;
    for (int32_t s : {(int32_t)n_a - 1, (int32_t)n_a}) lists.src.push_back(s);
    lists.end_row();
    for (int32_t s : {(int32_t)n_a, (int32_t)(n_a + n_b) - 1, (int32_t)n_a + 2}) lists.src.push_back(s);
    lists.end_row();
    for (int32_t s : {0, 5, 2, 2}) lists.src.push_back(s);
    lists.end_row();
    lists.end_row();
    for (int32_t s : {0, 1}) lists.src.push_back(s);
    lists.end_row();
    for (int32_t s = 0; s < (int32_t)(n_a + n_b); s++) lists.src.push_back(s);
    lists.end_row();
    CHECK(lists.n_lists() == 6 && lists.width(3) == 0);
    const std::vector<uint8_t> bits6 = {1, 0, 1, 1, 0, 1};
    for (int with_pub = 0; with_pub < 2; with_pub++) {
        RowPlan p = lists;
        if (with_pub) p.pub_bit = bits6;
        CHECK(run2(A, B, p, L) == direct2(A, B, p, L));
    }
    // shared lists under different bases: list 4 (sources 0, 1) at base 0 (A alone), at n_a - 1 (straddles) and at
    // n_a + 3 (the base alone carries it into B, up to its last source); list 2 twice
    RowPlan p = lists;
    p.list_of = {4, 4, 4, 2, 2, 3, 0};
    p.base_of = {0, (int32_t)n_a - 1, (int32_t)n_a + 3, 0, (int32_t)n_a - 1, 7, 0};
    for (int with_pub = 0; with_pub < 2; with_pub++) {
        if (with_pub) p.pub_bit = {0, 1, 1, 0, 1, 1, 0};
        const std::vector<uint64_t> out = run2(A, B, p, L);
        CHECK(out == direct2(A, B, p, L));
        // by hand: row 1 is A's last source plus B's first, row 2 B's last two, row 5 the empty list
        for (int c = 0; c < L; c++) {
            const uint64_t pub1 = with_pub && c == L - 1 ? 1ull << 63 : 0;
            CHECK(out[1 * L + c] == A[(n_a - 1) * L + c] + B[c] + pub1);
            CHECK(out[2 * L + c] == B[3 * L + c] + B[4 * L + c] + pub1);
            CHECK(out[5 * L + c] == pub1);
        }
    }
    // n_a = 0: everything reads B; A is an empty allocation
    {
        const std::vector<uint64_t> none;
        RowPlan q;
        for (int32_t s : {0, 4, 1}) q.src.push_back(s);
        q.end_row();
        q.src.push_back(0);
        q.end_row();
        q.base_of = {0, 4};
        CHECK(run2(none, B, q, L) == direct2(none, B, q, L));
        const std::vector<uint64_t> out = run2(none, B, q, L);
        for (int c = 0; c < L; c++) CHECK(out[L + c] == B[4 * L + c]);
        // and n_b = 0: the one-array form
        RowPlan a1;
        for (int32_t s : {0, 5}) a1.src.push_back(s);
        a1.end_row();
        std::vector<uint64_t> o2 = run2(A, none, a1, L);
        for (size_t t = 0; t < o2.size(); t++) CHECK(o2[t] == rowsum_word(A.data(), a1, t, L));
    }
    // ---- what rowplan2_ok refuses ----
    {
        CHECK(rowplan2_ok(p, n_a, n_b));
        CHECK(!rowplan2_ok(p, n_a, n_b - 1) && !rowplan2_ok(p, n_a - 1, n_b));  // base n_a + 3 + source 1 is the last
        RowPlan bad = p;
        bad.base_of[2] = (int32_t)n_a + 4;  // base + src == n_a + n_b
        CHECK(!rowplan2_ok(bad, n_a, n_b));
        bad = p;
        bad.base_of[1] = -1;  // a negative base, though base + src stays in range
        CHECK(!rowplan2_ok(bad, n_a, n_b));
        bad = lists;
        bad.src[1] = (int32_t)(n_a + n_b);  // an index equal to n_a + n_b
        CHECK(!rowplan2_ok(bad, n_a, n_b));
        bad = lists;
        bad.src[0] = -1;
        CHECK(!rowplan2_ok(bad, n_a, n_b));
        CHECK(rowplan2_ok(RowPlan{}, 0, 0));
    }
}

// ---- the plan of a call over key tables, on plain bits: a bit is bit 63 of its word, so u64 sums are XORs ----
static std::vector<uint64_t> bits_of(const GcmElem &e) {
    std::vector<uint64_t> v(128);
    for (int i = 0; i < 128; i++) v[i] = (uint64_t)gcm_coef(e, i) << 63;
    return v;
}

static void plan_replay(uint64_t &seed) {
    const size_t n_keys = 2, n_powers = 4;
    const int tag_len = 12;
    // two tables of H^1 .. H^4, slot-major as the caller keeps them
    GcmElem H[2] = {{{next(seed), next(seed)}}, {{next(seed), next(seed)}}};
    std::vector<uint64_t> A;
    for (size_t s = 0; s < n_keys; s++) {
        GcmElem p = H[s];
        for (size_t k = 0; k < n_powers; k++, p = gcm_mul(p, H[s])) {
            const std::vector<uint64_t> b = bits_of(p);
            A.insert(A.end(), b.begin(), b.end());
        }
    }
    // three frames under slots 1, 0, 1 with m = 1, 2, 4
    const uint8_t iv[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    uint8_t aad[8], data[20], tags[3][12];
    for (auto &b : aad) b = (uint8_t)next(seed);
    for (auto &b : data) b = (uint8_t)next(seed);
    for (auto &t : tags)
        for (auto &b : t) b = (uint8_t)next(seed);
    std::vector<GcmFrame> frames(3);
    CHECK(gcm_format(iv, 12, nullptr, 0, nullptr, 0, tag_len, frames[0]) == GCM_FMT_OK);
    CHECK(gcm_format(iv, 12, aad, 5, nullptr, 0, tag_len, frames[1]) == GCM_FMT_OK);
    CHECK(gcm_format(iv, 12, aad, 8, data, 20, tag_len, frames[2]) == GCM_FMT_OK);
    CHECK(frames[0].m() == 1 && frames[1].m() == 2 && frames[2].m() == 4);
    const size_t slots[3] = {1, 0, 1};
    std::vector<uint64_t> B;  // E(J0) of every frame: arbitrary bits
    GcmElem j0[3];
    for (auto &e : j0) {
        e = GcmElem{{next(seed), next(seed)}};
        const std::vector<uint64_t> b = bits_of(e);
        B.insert(B.end(), b.begin(), b.end());
    }
    CHECK(gcm_multi_shape_ok(n_keys, n_powers, 3));
    GcmCallPlan multi;
    std::vector<std::vector<int32_t>> rows;
    for (size_t f = 0; f < 3; f++) {
        gcm_frame_rows(frames[f], rows);
        CHECK(gcm_multi_frame_check(frames[f], (int64_t)slots[f], n_keys, n_powers, tag_len, rows) == GCM_MULTI_OK);
        gcm_multi_plan_add(multi, rows, n_keys, n_powers, slots[f], f, tags[f]);
    }
    CHECK(multi.chunks.base_of.size() == multi.chunks.n_rows() && multi.chunks.list_of.empty());
    // the largest index is E(J0) bit 8 tag_len - 1 of the last frame
    CHECK(rowplan2_ok(multi.chunks, A.size(), B.size()) && rowplan2_ok(multi.chunks, A.size(), 2 * 128 + 96) &&
          !rowplan2_ok(multi.chunks, A.size(), 2 * 128 + 95));
    const std::vector<uint64_t> chunks = run2(A, B, multi.chunks, 1);
    std::vector<uint64_t> diff(multi.diff.n_rows());
    CHECK(rowplan_ok(multi.diff, chunks.size()));
    for (size_t t = 0; t < diff.size(); t++) diff[t] = rowsum_word(chunks.data(), multi.diff, t, 1);
    CHECK(diff.size() == 3 * 8 * (size_t)tag_len);

    size_t chunk_at = 0;
    for (size_t f = 0; f < 3; f++) {
        // the single-key call of this frame alone on its slot's table: the table's first m blocks, then E(J0)
        const size_t m = frames[f].m();
        std::vector<uint64_t> src(A.begin() + (std::ptrdiff_t)(slots[f] * n_powers * 128),
                                  A.begin() + (std::ptrdiff_t)((slots[f] * n_powers + m) * 128));
        src.insert(src.end(), B.begin() + (std::ptrdiff_t)(f * 128), B.begin() + (std::ptrdiff_t)((f + 1) * 128));
        GcmCallPlan one;
        gcm_frame_rows(frames[f], rows);
        gcm_call_plan_add(one, rows, m, 0, tags[f]);
        CHECK(rowplan_ok(one.chunks, src.size()));
        std::vector<uint64_t> c1(one.chunks.n_rows()), d1(one.diff.n_rows());
        for (size_t t = 0; t < c1.size(); t++) c1[t] = rowsum_word(src.data(), one.chunks, t, 1);
        for (size_t t = 0; t < d1.size(); t++) d1[t] = rowsum_word(c1.data(), one.diff, t, 1);
        for (size_t t = 0; t < c1.size(); t++) CHECK(chunks[chunk_at + t] == c1[t]);
        chunk_at += c1.size();
        for (size_t t = 0; t < d1.size(); t++) CHECK(diff[f * d1.size() + t] == d1[t]);
        // and GHASH itself: sum X_i H^(m + 1 - i) + E(J0) + the received tag
        GcmElem g{{0, 0}}, p = H[slots[f]];
        for (size_t k = 1; k <= m; k++, p = gcm_mul(p, H[slots[f]])) {
            const GcmElem t = gcm_mul(gcm_from_bytes(&frames[f].hashed[(m - k) * 16]), p);
            g.w[0] ^= t.w[0];
            g.w[1] ^= t.w[1];
        }
        g.w[0] ^= j0[f].w[0];
        g.w[1] ^= j0[f].w[1];
        uint8_t gb[16];
        gcm_to_bytes(g, gb);
        for (int r = 0; r < 8 * tag_len; r++) {
            const uint64_t want = (uint64_t)(((gb[r >> 3] ^ tags[f][r >> 3]) >> (7 - (r & 7))) & 1) << 63;
            CHECK(d1[(size_t)r] == want);
        }
    }
    CHECK(chunk_at == chunks.size());

    // ---- what a call refuses, per frame ----
    gcm_frame_rows(frames[2], rows);
    CHECK(gcm_multi_frame_check(frames[2], 2, n_keys, n_powers, tag_len, rows) == GCM_MULTI_SLOT);
    CHECK(gcm_multi_frame_check(frames[2], -1, n_keys, n_powers, tag_len, rows) == GCM_MULTI_SLOT);
    CHECK(gcm_multi_frame_check(frames[2], 1, n_keys, 3, tag_len, rows) == GCM_MULTI_POWERS);
    CHECK(gcm_multi_frame_check(frames[2], 1, n_keys, n_powers, 16, rows) == GCM_MULTI_TAG);  // mixed tag lengths
    CHECK(!gcm_multi_shape_ok(n_keys, 0, 1) && !gcm_multi_shape_ok(n_keys, 65, 1) && !gcm_multi_shape_ok(65537, 4, 1));
}

int main() {
    uint64_t seed = 0x13198a2e03707344ULL;
    word_cases(3, seed);
    word_cases(2049, seed);
    plan_replay(seed);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
