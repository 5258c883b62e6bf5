// The GCM host layer (csrc/aes_gcm.hpp) compiled stand-alone, on PLAIN BIT VALUES: a "ciphertext" is L = 3 words
// whose body word holds the bit at 1 << 63, sums are the u64 additions rowsum_word does, a refresh is the identity
// on the bit (the body's top bit) and the 8 -> 7 table is evaluated directly.  Checked against the bitwise product of
// SP 800-38D algorithm 1: the power schedule H^1 .. H^5 of test case 2's H, products with 0, 1, x^127 and all-ones,
// the tag difference of test case 4 and of a one-bit-flipped tag, and the one-slot plan of a two-frame call over a
// table and E(J0) blocks in separate exact allocations (rowsum2_word).  Built and run by tests/test_aes_gcm.py, also
// under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/aes_gcm.hpp"

using namespace tae;

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                \
        }                                                           \
    } while (0)

static const int L = 3;
using Cts = std::vector<uint64_t>;  // [n][L]

static Cts encode(const GcmElem &a) {
    Cts c((size_t)128 * L, 0);
    for (int k = 0; k < 128; k++) {
        c[(size_t)k * L] = 0x1111 * (uint64_t)(k + 1);  // mask words: the sums must carry them along untouched
        c[(size_t)k * L + L - 1] = (uint64_t)gcm_coef(a, k) << 63;
    }
    return c;
}

static GcmElem decode(const uint64_t *c) {
    GcmElem a{{0, 0}};
    for (int k = 0; k < 128; k++)
        if (c[(size_t)k * L + L - 1] >> 63) a.w[k >> 6] |= 1ull << (63 - (k & 63));
    return a;
}

static Cts rowsum(const Cts &src, const RowPlan &p) {
    CHECK(rowplan_ok(p, src.size() / L));
    Cts out(p.n_rows() * L);
    for (size_t t = 0; t < out.size(); t++) out[t] = rowsum_word(src.data(), p, t, L);
    return out;
}

// the square plan reading block `block` of the source array
static RowPlan square_of(size_t block) {
    RowPlan p = gcm_square_plan();
    p.base_of.assign(128, (int32_t)(block * 128));
    return p;
}

// the identity bootstrap: the bit survives, the rest is new
static Cts refresh(const Cts &in) {
    Cts out(in.size(), 0);
    for (size_t i = 0; i < in.size() / L; i++) out[i * L + L - 1] = in[i * L + L - 1] & (1ull << 63);
    return out;
}

static bool eq(const GcmElem &a, const GcmElem &b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1]; }

// one product through the plan: pairs, the table, chunk sums, refresh, reduction, refresh
static GcmElem product(const GcmElem &a, const GcmElem &b, const GcmProductPlan &P) {
    Cts parts((size_t)kGcmParts * L, 0);
    for (int g = 0; g < kGcmGroups; g++) {
        unsigned v = 0;
        for (int bit = 0; bit < 8; bit++) {
            const int s = gcm_pair_source(g, bit);
            v = (v << 1) | (unsigned)(s < 128 ? gcm_coef(a, s) : gcm_coef(b, s - 128));
        }
        const uint64_t f = gcm_nibble_product(v);
        for (int d = 0; d < kGcmPartBits; d++)
            parts[((size_t)g * kGcmPartBits + d) * L + L - 1] = ((f >> (kGcmPartBits - 1 - d)) & 1) << 63;
    }
    const Cts chunks = refresh(rowsum(parts, P.chunks));
    const Cts red = refresh(rowsum(chunks, P.reduce));
    return decode(red.data());
}

static GcmElem hex(const char *s) {
    uint8_t b[16];
    for (int i = 0; i < 16; i++) {
        unsigned v;
        std::sscanf(s + 2 * i, "%2x", &v);
        b[i] = (uint8_t)v;
    }
    return gcm_from_bytes(b);
}

static std::vector<uint8_t> bytes(const char *s) {
    std::vector<uint8_t> v(std::strlen(s) / 2);
    for (size_t i = 0; i < v.size(); i++) {
        unsigned x;
        std::sscanf(s + 2 * i, "%2x", &x);
        v[i] = (uint8_t)x;
    }
    return v;
}

int main() {
    // ---- the field ----
    const GcmElem one = gcm_x_pow(0), H = hex("66e94bd4ef8a2c3b884cfa59ca342b2e");
    const GcmElem zero{{0, 0}}, ones{{~0ull, ~0ull}}, top = gcm_x_pow(127);
    uint8_t b16[16];
    gcm_to_bytes(gcm_times_x(top), b16);
    CHECK(b16[0] == 0xE1 && b16[15] == 0);  // x^128 = 1 + x + x^2 + x^7
    CHECK(eq(gcm_mul(H, one), H) && eq(gcm_mul(one, H), H) && eq(gcm_mul(H, zero), zero));
    CHECK(eq(gcm_mul(H, ones), gcm_mul(ones, H)));
    GcmElem cols[128];
    gcm_mul_cols(H, cols);
    CHECK(eq(cols[0], H) && eq(cols[127], gcm_mul(H, top)));

    // ---- the product plan ----
    const GcmProductPlan P = gcm_product_plan();
    CHECK(P.chunks.src.size() == 7168 && P.chunks.n_rows() == 1135 && P.chunks.max_width() == 7);
    CHECK(P.reduce.n_rows() == 128 && P.reduce.max_width() <= 34);
    const GcmElem ops[] = {zero, one, top, ones, H};
    for (const GcmElem &a : ops)
        for (const GcmElem &b : ops) CHECK(eq(product(a, b, P), gcm_mul(a, b)));

    // ---- the power schedule on plain bits: H^1 .. H^5 ----
    const std::vector<GcmGeneration> gens = gcm_power_schedule(5);
    CHECK(gens.size() == 3 && gens[0].squares == std::vector<int>{2} && gens[1].products == std::vector<int>{3} &&
          gens[1].squares == std::vector<int>{4} && gens[2].products == std::vector<int>{5});
    Cts table((size_t)5 * 128 * L, 0);
    auto put = [&](int k, const Cts &c) { std::memcpy(&table[(size_t)(k - 1) * 128 * L], c.data(), c.size() * 8); };
    put(1, refresh(encode(H)));
    for (const GcmGeneration &g : gens) {
        for (int k : g.squares) put(k, refresh(rowsum(table, square_of((size_t)(k / 2 - 1)))));
        for (int k : g.products)
            put(k, encode(product(decode(&table[(size_t)(k - 2) * 128 * L]), decode(table.data()), P)));
    }
    GcmElem want = H;
    for (int k = 1; k <= 5; k++, want = gcm_mul(want, H)) CHECK(eq(decode(&table[(size_t)(k - 1) * 128 * L]), want));
    CHECK(gcm_square_plan().max_width() <= 5);
    // 15 = ((2 . 2 + 1) . 2 + 1) . 2 + 1 is the deepest of 16: square, product, square, product, square, product
    CHECK(gcm_power_schedule(16).size() == 6 && gcm_power_schedule(1).empty());

    // ---- the frame plan: test case 4 ----
    const std::vector<uint8_t> iv = bytes("cafebabefacedbaddecaf888"), aad = bytes("feedfacedeadbeeffeedfacedeadbeefabaddad2");
    const std::vector<uint8_t> ct = bytes("42831ec2217774244b7221b784d0d49ce3aa212f2c02a4e035c17e2329aca12e"
                                          "21d514b25466931c7d8f6a5aac84aa051ba30b396a0aac973d58e091");
    const std::vector<uint8_t> tag = bytes("5bc94fbc3221a5db94fae95ae7121a47");
    const GcmElem H4 = hex("b83b533708bf535d0aa6e52980d53b78"), EJ0 = hex("3247184b3c4f69a44dbcd22887bbb418");
    GcmFrame f;
    CHECK(gcm_format(iv.data(), 12, aad.data(), aad.size(), ct.data(), ct.size(), 16, f) == GCM_FMT_OK);
    CHECK(f.m() == 7 && f.n_pub() == 6);
    CHECK(f.pub[16 + 15] == 1 && f.pub[32 + 15] == 2 && f.pub[5 * 16 + 15] == 5 && f.pub[0] == 0 && f.pub[16] == 0xca);
    CHECK(f.hashed[6 * 16 + 7] == 0xa0 && f.hashed[6 * 16 + 14] == 0x01 && f.hashed[6 * 16 + 15] == 0xe0);
    CHECK(f.hashed[16 + 4] == 0 && f.hashed[5 * 16 + 12] == 0);  // the paddings
    std::vector<std::vector<int32_t>> rows;
    gcm_frame_rows(f, rows);
    CHECK(rows.size() == 128 && gcm_frame_check(f, 7, rows) == GCM_PLAN_OK && gcm_frame_check(f, 6, rows) == GCM_PLAN_POWERS);
    // sources: the table H^1 .. H^7 (plain powers), then E(J0)
    Cts src;
    GcmElem p = H4;
    for (int k = 1; k <= 7; k++, p = gcm_mul(p, H4)) {
        const Cts e = encode(p);
        src.insert(src.end(), e.begin(), e.end());
    }
    const Cts ej = encode(EJ0);
    src.insert(src.end(), ej.begin(), ej.end());
    for (int flip = 0; flip < 2; flip++) {
        std::vector<uint8_t> t = tag;
        if (flip) t[13] ^= 0x04;  // tag bit 13 * 8 + 5
        GcmCallPlan plan;
        gcm_call_plan_add(plan, rows, 7, 0, t.data());
        CHECK(plan.chunks.max_width() <= 64 && plan.diff.n_rows() == 128 && plan.chunks_of_row.size() == 128);
        for (size_t r = 0; r < 128; r++) {
            CHECK((size_t)plan.chunks_of_row[r] == gcm_row_chunks(rows[r].size()));
            CHECK(plan.diff.width(r) == plan.chunks_of_row[r]);
        }
        const Cts diff = rowsum(refresh(rowsum(src, plan.chunks)), plan.diff);
        const GcmElem d = decode(diff.data());
        GcmElem wantd{{0, 0}};
        if (flip) wantd.w[1] = 1ull << (63 - (13 * 8 + 5 - 64));
        CHECK(eq(d, wantd));
    }
    // the first chunk has room for 55 sources next to E(J0), later ones for 64
    CHECK(gcm_row_chunks(0) == 1 && gcm_row_chunks(55) == 1 && gcm_row_chunks(56) == 2 && gcm_row_chunks(55 + 64) == 2 &&
          gcm_row_chunks(55 + 65) == 3);
    // an empty frame: one all-zero length block, every row its E(J0) bit alone
    GcmFrame e;
    CHECK(gcm_format(iv.data(), 12, nullptr, 0, nullptr, 0, 4, e) == GCM_FMT_OK && e.m() == 1 && e.n_pub() == 2);
    gcm_frame_rows(e, rows);
    CHECK(rows.size() == 32);
    for (const auto &r : rows) CHECK(r.empty());
    CHECK(gcm_format(iv.data(), 16, nullptr, 0, nullptr, 0, 16, e) == GCM_FMT_IV);
    CHECK(gcm_format(iv.data(), 12, nullptr, 0, nullptr, 0, 5, e) == GCM_FMT_TAG);
    // ---- the one-slot plan of a call: a table of 4 powers, frames of m = 1 and m = 2.  A is the table
    // and B the E(J0) blocks, each a heap allocation of exactly its size, so the sanitized build reports an index past
    // either end.  E(J0) of frame f is source (n_powers + f) 128 + r whatever the frames' m is ----
    {
        const size_t n_powers = 4, n_a = n_powers * 128, n_b = 2 * 128;
        const int tl = 8;
        std::unique_ptr<uint64_t[]> A(new uint64_t[n_a * L]), B(new uint64_t[n_b * L]);
        GcmElem pw = H4;
        for (size_t k = 0; k < n_powers; k++, pw = gcm_mul(pw, H4)) {
            const Cts c = refresh(encode(pw));
            std::memcpy(&A[k * 128 * L], c.data(), c.size() * 8);
        }
        const GcmElem j0[2] = {EJ0, gcm_mul(EJ0, H)};
        for (size_t fi = 0; fi < 2; fi++) {
            const Cts c = encode(j0[fi]);
            std::memcpy(&B[fi * 128 * L], c.data(), c.size() * 8);
        }
        GcmFrame fr[2];
        CHECK(gcm_format(iv.data(), 12, nullptr, 0, nullptr, 0, tl, fr[0]) == GCM_FMT_OK && fr[0].m() == 1);
        CHECK(gcm_format(iv.data(), 12, nullptr, 0, ct.data(), 9, tl, fr[1]) == GCM_FMT_OK && fr[1].m() == 2);
        const uint8_t tags[2][8] = {{0x5b, 0xc9, 0x4f, 0xbc, 0x32, 0x21, 0xa5, 0xdb}, {0x94, 0xfa, 0xe9, 0x5a, 0xe7, 0x12, 0x1a, 0x47}};
        CHECK(gcm_plan_index_ok(1, n_powers, 2) && gcm_plan_index_ok(1, 128, 1) && !gcm_plan_index_ok(1, (size_t)1 << 24, 1) &&
              !gcm_plan_index_ok((size_t)1 << 12, (size_t)1 << 12, 1));
        GcmCallPlan plan;
        for (size_t fi = 0; fi < 2; fi++) {
            gcm_frame_rows(fr[fi], rows);
            CHECK(gcm_multi_frame_check(fr[fi], 0, 1, n_powers, tl, rows) == GCM_MULTI_OK);
            gcm_multi_plan_add(plan, rows, 1, n_powers, 0, fi, tags[fi]);
        }
        // the largest index is bit 8 tl - 1 of the last frame's E(J0); row 0 of frame 1 starts with its E(J0) bit 0
        CHECK(rowplan2_ok(plan.chunks, n_a, n_b) && rowplan2_ok(plan.chunks, n_a, 128 + 64) && !rowplan2_ok(plan.chunks, n_a, 128 + 63));
        CHECK(plan.chunks.src[(size_t)plan.chunks.row_start[(size_t)8 * tl]] == (int32_t)((n_powers + 1) * 128));
        Cts chunks(plan.chunks.n_rows() * L);
        for (size_t t = 0; t < chunks.size(); t++) chunks[t] = rowsum2_word(A.get(), n_a, B.get(), plan.chunks, t, L);
        const Cts diff = rowsum(refresh(chunks), plan.diff);
        CHECK(diff.size() == (size_t)2 * 8 * tl * L);
        for (size_t fi = 0; fi < 2; fi++) {
            GcmElem y{{0, 0}};  // GHASH by Horner's rule, then E(J0) and the received tag
            for (size_t i = 0; i < fr[fi].m(); i++) {
                const GcmElem x = gcm_from_bytes(&fr[fi].hashed[16 * i]);
                y = gcm_mul(GcmElem{{y.w[0] ^ x.w[0], y.w[1] ^ x.w[1]}}, H4);
            }
            uint8_t tb[16] = {0};
            std::memcpy(tb, tags[fi], 8);
            const GcmElem t = gcm_from_bytes(tb);
            const GcmElem wantd{{y.w[0] ^ j0[fi].w[0] ^ t.w[0], y.w[1] ^ j0[fi].w[1] ^ t.w[1]}};
            for (int r = 0; r < 8 * tl; r++)
                CHECK((int)(diff[(fi * 8 * tl + (size_t)r) * L + L - 1] >> 63) == gcm_coef(wantd, r));
        }
    }
    // a broken plan is refused before a launch
    RowPlan bad = P.reduce;
    bad.src[3] = 1135;
    CHECK(!rowplan_ok(bad, 1135) && rowplan_ok(P.reduce, 1135));
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
