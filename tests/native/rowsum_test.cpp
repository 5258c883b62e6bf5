// Host check of the row-sum layer (csrc/rowsum.hpp), the arithmetic of the device kernel on plain words at L = 3:
// rowsum_word with every nullable argument taken both ways (list_of null / shared lists, base_of null / non-zero,
// pub_bit null / present) against a direct double loop, an empty list and a list of width 64 among them; what
// rowplan_ok refuses; and a plan repeated through list_of / base_of against the explicit copy of its lists, on GCM's
// reduction plan.  Stand-alone: built plain and with -fsanitize=address,undefined by tests/test_rowsum.py.
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

static const int L = 3;

static uint64_t next(uint64_t &seed) {
    seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
    return seed ^ (seed >> 29);
}

// every word through rowsum_word
static std::vector<uint64_t> run(const std::vector<uint64_t> &src, const RowPlan &p) {
    CHECK(rowplan_ok(p, src.size() / L));
    std::vector<uint64_t> out(p.n_rows() * L);
    for (size_t t = 0; t < out.size(); t++) out[t] = rowsum_word(src.data(), p, t, L);
    return out;
}

// the definition, row by row and source by source
static std::vector<uint64_t> direct(const std::vector<uint64_t> &src, const RowPlan &p) {
    std::vector<uint64_t> out(p.n_rows() * L, 0);
    for (size_t r = 0; r < p.n_rows(); r++) {
        const size_t l = p.list_of.empty() ? r : (size_t)p.list_of[r], base = p.base_of.empty() ? 0 : (size_t)p.base_of[r];
        for (int32_t q = p.row_start[l]; q < p.row_start[l + 1]; q++)
            for (int c = 0; c < L; c++) out[r * L + c] += src[(base + (size_t)p.src[q]) * L + c];
        if (!p.pub_bit.empty()) out[r * L + L - 1] += (uint64_t)p.pub_bit[r] << 63;
    }
    return out;
}

// `count` explicit copies of a plan's lists, copy c reading its sources at + c * src_stride: what the shared lists
// replace
static RowPlan explicit_copies(const RowPlan &p, size_t count, size_t src_stride) {
    RowPlan out;
    for (size_t c = 0; c < count; c++)
        for (size_t r = 0; r < p.n_lists(); r++) {
            for (int32_t q = p.row_start[r]; q < p.row_start[r + 1]; q++)
                out.src.push_back(p.src[q] + (int32_t)(c * src_stride));
            out.end_row();
        }
    return out;
}

int main() {
    uint64_t seed = 0x243f6a8885a308d3ULL;
    const size_t block = 70, n_src = 3 * block;  // three "units" of 70 sources
    std::vector<uint64_t> src(n_src * L);
    for (auto &w : src) w = next(seed);  // full words: the sums wrap

    // five lists over one unit: width 1, empty, width 64, width 7 with a repeated source, the last source alone
    RowPlan lists;
    lists.src.push_back(5);
    lists.end_row();
    lists.end_row();
    for (int i = 0; i < 64; i++) lists.src.push_back((int32_t)((i * 37 + 11) % block));
    lists.end_row();
    for (int32_t s : {3, 9, 3, 69, 0, 41, 12}) lists.src.push_back(s);
    lists.end_row();
    lists.src.push_back((int32_t)block - 1);
    lists.end_row();
    CHECK(lists.n_lists() == 5 && lists.n_rows() == 5 && lists.width(1) == 0 && lists.max_width() == 64);

    // the shared-list form: 8 rows, lists read twice under one base and under three bases
    const std::vector<int32_t> list_of = {2, 0, 2, 4, 1, 3, 3, 4}, base_of = {0, 70, 140, 140, 70, 0, 70, 0};
    const std::vector<uint8_t> bits8 = {1, 0, 0, 1, 1, 0, 1, 0}, bits5 = {0, 1, 1, 0, 1};
    for (int with_list = 0; with_list < 2; with_list++)
        for (int with_base = 0; with_base < 2; with_base++)
            for (int with_pub = 0; with_pub < 2; with_pub++) {
                RowPlan p = lists;
                if (with_list) p.list_of = list_of;
                if (with_base) p.base_of = with_list ? base_of : std::vector<int32_t>{140, 0, 70, 70, 140};
                if (with_pub) p.pub_bit = with_list ? bits8 : bits5;
                CHECK(p.n_rows() == (with_list ? 8u : 5u));
                CHECK(run(src, p) == direct(src, p));
            }
    {
        // the words themselves, once by hand: row 3 of the shared form is list 4 (source 69) at base 140, bit 1
        RowPlan p = lists;
        p.list_of = list_of;
        p.base_of = base_of;
        p.pub_bit = bits8;
        const std::vector<uint64_t> out = run(src, p);
        for (int c = 0; c < L; c++)
            CHECK(out[3 * L + c] == src[(140 + 69) * L + c] + (c == L - 1 ? 1ull << 63 : 0));
        for (int c = 0; c < L; c++) CHECK(out[4 * L + c] == (c == L - 1 ? 1ull << 63 : 0));  // the empty list
    }

    // ---- what rowplan_ok refuses ----
    {
        RowPlan ok = lists;
        ok.list_of = list_of;
        ok.base_of = base_of;
        ok.pub_bit = bits8;
        CHECK(rowplan_ok(ok, n_src));
        CHECK(!rowplan_ok(ok, n_src - 1));  // base 140 + source 69 == n_src - 1 is the last source
        RowPlan bad = ok;
        bad.list_of[5] = 5;  // a list_of out of range
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.list_of[5] = -1;
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.base_of[3] = 141;  // base + src == n_src
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.base_of[1] = -70;
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.row_start[2] = 0;  // a decreasing row_start
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.row_start[2] = 1000;  // decreasing after an entry past src: refused before that list is walked
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.row_start.back()--;  // not whole lists
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.src[7] = -1;
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.pub_bit[2] = 2;  // a pub_bit of 2
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.pub_bit.pop_back();  // a pub_bit array of the wrong length
        CHECK(!rowplan_ok(bad, n_src));
        bad = ok;
        bad.base_of.push_back(0);
        CHECK(!rowplan_ok(bad, n_src));
        bad = lists;  // without list_of the rows are the lists: five bits, five bases
        bad.pub_bit = bits8;
        CHECK(!rowplan_ok(bad, n_src));
        bad = lists;
        bad.base_of = base_of;
        CHECK(!rowplan_ok(bad, n_src));
        CHECK(rowplan_ok(lists, block) && !rowplan_ok(lists, block - 1));
        CHECK(rowplan_ok(RowPlan{}, 0));  // no rows: nothing to launch
    }

    // ---- a plan repeated through list_of / base_of equals the explicit copy of its lists: GCM's reduction ----
    {
        const GcmProductPlan P = gcm_product_plan();
        const size_t n_chunks = P.chunks.n_rows(), count = 3;
        // `count` copies read their own sources
        const RowPlan rep = explicit_copies(P.reduce, 2, P.chunks.n_rows());
        CHECK(rep.n_rows() == 256 && rep.src[P.reduce.src.size()] == P.reduce.src[0] + 1135);
        std::vector<uint64_t> chunks(count * n_chunks * L);
        for (auto &w : chunks) w = next(seed);
        RowPlan shared = P.reduce;
        for (size_t r = 0; r < count * 128; r++) {
            shared.list_of.push_back((int32_t)(r % 128));
            shared.base_of.push_back((int32_t)(r / 128 * n_chunks));
        }
        const RowPlan copies = explicit_copies(P.reduce, count, n_chunks);
        CHECK(shared.n_rows() == copies.n_rows() && shared.src.size() * count == copies.src.size());
        CHECK(run(chunks, shared) == run(chunks, copies));
        CHECK(rowplan_ok(shared, count * n_chunks - 1) == rowplan_ok(copies, count * n_chunks - 1));
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
