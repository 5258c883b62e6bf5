// AES-GCM (NIST SP 800-38D) decryption of a public frame under FHE: the field, the row-sum plans and the frame
// layout.  Plain C++ in the style of aes_xts.hpp and aes_ccm.hpp: the plans have no device code and
// the row sums are rowsum.hpp's, host/device, so a stand-alone program runs the whole algorithm on plain bits
// (tests/native/aes_gcm_test.cpp).
//
//   H = E_K(0^128)    J0 = iv || 00000001    P_i = C_i ^ E_K(iv || be32(2 + i))
//   tag = E_K(J0) ^ GHASH,   GHASH = sum_{i = 1..m} X_i H^(m + 1 - i)
//
// X_1 .. X_m are the zero-padded AAD, the zero-padded ciphertext and be64(8 |aad|) || be64(8 |C|): all public.  So
// "X times an encrypted value" is a GF(2) matrix on the value's bits, an LWE row sum on ciphertexts, and the only
// products of two encrypted values are those of the power table H^1 .. H^n, made once per key.
//
// GCM's field is bit-reflected: the coefficient of x^k is bit k counted from the MSB of byte 0.  The project stores
// bytes MSB first, so coefficient k is ciphertext k of a block (aes_xts.hpp differs).  "Times x" is a right shift of
// the 128-bit string with 0xE1 into byte 0 on carry out: x^128 = 1 + x + x^2 + x^7.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rowsum.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TAE_GCM_HD __host__ __device__ inline
#else
#define TAE_GCM_HD inline
#endif

namespace tae {

// ---- the field ----
// coefficient k is bit 63 - (k & 63) of w[k >> 6]: byte 0 of the block is the top byte of w[0]
struct GcmElem {
    uint64_t w[2];
};

inline int gcm_coef(const GcmElem &a, int k) { return (int)((a.w[k >> 6] >> (63 - (k & 63))) & 1); }

inline GcmElem gcm_from_bytes(const uint8_t b[16]) {
    GcmElem a{{0, 0}};
    for (int i = 0; i < 16; i++) a.w[i >> 3] |= (uint64_t)b[i] << (56 - 8 * (i & 7));
    return a;
}

inline void gcm_to_bytes(const GcmElem &a, uint8_t b[16]) {
    for (int i = 0; i < 16; i++) b[i] = (uint8_t)(a.w[i >> 3] >> (56 - 8 * (i & 7)));
}

inline GcmElem gcm_times_x(GcmElem a) {
    const uint64_t carry = a.w[1] & 1;
    a.w[1] = (a.w[1] >> 1) | (a.w[0] << 63);
    a.w[0] = (a.w[0] >> 1) ^ (carry ? 0xE1ull << 56 : 0);
    return a;
}

// SP 800-38D algorithm 1, bit by bit
inline GcmElem gcm_mul(const GcmElem &x, GcmElem v) {
    GcmElem z{{0, 0}};
    for (int i = 0; i < 128; i++, v = gcm_times_x(v))
        if (gcm_coef(x, i)) {
            z.w[0] ^= v.w[0];
            z.w[1] ^= v.w[1];
        }
    return z;
}

// x^t, stepped (t <= 254 here)
inline GcmElem gcm_x_pow(int t) {
    GcmElem r{{1ull << 63, 0}};
    while (t-- > 0) r = gcm_times_x(r);
    return r;
}

// the column images of "multiply by the public X": cols[i] = X x^i, stepped as xts_rows_of does
inline void gcm_mul_cols(GcmElem X, GcmElem cols[128]) {
    for (int i = 0; i < 128; i++, X = gcm_times_x(X)) cols[i] = X;
}

// ---- squaring: linear over GF(2).  Row r lists the bits i of the operand with x^(2 i) mod p containing x^r; the
// operand is block 0 of the source array (another block: base_of = 128 block) ----
inline RowPlan gcm_square_plan() {
    RowPlan p;
    GcmElem sq[128];
    for (int i = 0; i < 128; i++) sq[i] = gcm_x_pow(2 * i);
    for (int r = 0; r < 128; r++) {
        for (int i = 0; i < 128; i++)
            if (gcm_coef(sq[i], r)) p.src.push_back((int32_t)i);
        p.end_row();
    }
    return p;
}

// ---- the product of two encrypted elements: 32 x 32 nibble pairs through one 8 -> 7 table ----
constexpr int kGcmGroups = 1024;      // group g = 32 I + J: bits 4I .. 4I+3 of a, bits 4J .. 4J+3 of b
constexpr int kGcmPartBits = 7;       // output d of a group: unreduced coefficient 4I + 4J + d
constexpr int kGcmParts = kGcmGroups * kGcmPartBits;
constexpr int kGcmChunkBits = 7;      // partial bits (level 8) per refreshed chunk: 7 * 8 = 56 <= 64

// The table: v = the group's 8 input bits, MSB first (a's four, then b's four; within a nibble the first bit is the
// lowest coefficient).  The value holds coefficient d of the carry-less product at bit 6 - d, so output d of the
// circuit bootstrap is coefficient d.
inline uint64_t gcm_nibble_product(unsigned v) {
    uint64_t r = 0;
    for (int p = 0; p < 4; p++)
        for (int q = 0; q < 4; q++)
            if (((v >> (7 - p)) & 1) && ((v >> (3 - q)) & 1)) r ^= 1ull << (6 - (p + q));
    return r;
}

// operand ciphertext of input `bit` (0..7) of group g, among the 256 operand bits a[0..128) b[0..128) of a product
TAE_GCM_HD int gcm_pair_source(int g, int bit) {
    return bit < 4 ? 4 * (g >> 5) + bit : 128 + 4 * (g & 31) + (bit - 4);
}

struct GcmProductPlan {
    RowPlan chunks;            // over the partial bits [1024][7]: greedy chunks of at most 7 per coefficient t
    std::vector<int> chunk_t;  // the unreduced coefficient (0 .. 254) of every chunk
    RowPlan reduce;            // over the refreshed chunks: bit r sums the chunks of every t with x^t mod p containing x^r
};

inline GcmProductPlan gcm_product_plan() {
    GcmProductPlan P;
    for (int t = 0; t < 255; t++) {
        int in_chunk = 0;
        for (int g = 0; g < kGcmGroups; g++) {  // ascending group order
            const int d = t - 4 * (g >> 5) - 4 * (g & 31);
            if (d < 0 || d >= kGcmPartBits) continue;
            if (in_chunk == kGcmChunkBits) {
                P.chunks.end_row();
                P.chunk_t.push_back(t);
                in_chunk = 0;
            }
            P.chunks.src.push_back(g * kGcmPartBits + d);
            in_chunk++;
        }
        if (in_chunk) {
            P.chunks.end_row();
            P.chunk_t.push_back(t);
        }
    }
    GcmElem xt[255];
    xt[0] = gcm_x_pow(0);
    for (int t = 1; t < 255; t++) xt[t] = gcm_times_x(xt[t - 1]);
    for (int r = 0; r < 128; r++) {
        for (size_t c = 0; c < P.chunk_t.size(); c++)
            if (gcm_coef(xt[P.chunk_t[c]], r)) P.reduce.src.push_back((int32_t)c);
        P.reduce.end_row();
    }
    return P;
}

// ---- the power schedule: H^1 is the refreshed E_K(0); an even power is the square of H^(k/2) (row sums, then a
// refresh), an odd one the product H^(k-1) H.  A generation's squares share one launch sequence, its products another ----
struct GcmGeneration {
    std::vector<int> squares, products;  // the powers k made in this generation
};

inline std::vector<GcmGeneration> gcm_power_schedule(int n_powers) {
    std::vector<int> gen((size_t)n_powers + 1, 0);
    std::vector<GcmGeneration> out;
    for (int k = 2; k <= n_powers; k++) {
        gen[k] = 1 + ((k & 1) ? gen[k - 1] : gen[k / 2]);
        if ((size_t)gen[k] > out.size()) out.resize(gen[k]);
    }
    for (int k = 2; k <= n_powers; k++) ((k & 1) ? out[gen[k] - 1].products : out[gen[k] - 1].squares).push_back(k);
    return out;
}

constexpr int kGcmMaxPowers = 64;  // a frame's rows refuse more hashed blocks than that anyway

// ---- the frame ----
struct GcmFrame {
    int tag_len = 0;
    size_t aad_len = 0, data_len = 0;
    std::vector<uint8_t> pub;     // [2 + ceil(data_len / 16)][16]: 0^128 (the key's H), J0, iv || be32(2 + i)
    std::vector<uint8_t> hashed;  // [m][16]: X_1 .. X_m
    size_t n_pub() const { return pub.size() / 16; }
    size_t m() const { return hashed.size() / 16; }
};

enum GcmFormat { GCM_FMT_OK = 0, GCM_FMT_IV, GCM_FMT_TAG };

inline bool gcm_tag_len_ok(int t) { return t == 4 || t == 8 || (t >= 12 && t <= 16); }

// Only 96-bit IVs: another length needs GHASH over the IV.  aad / data may be null when their length is 0.  The low 32
// bits of the counter wrap modulo 2^32 and never carry into the IV.  On an error the frame is left empty.
inline GcmFormat gcm_format(const uint8_t *iv, size_t iv_len, const uint8_t *aad, size_t aad_len, const uint8_t *data,
                            size_t data_len, int tag_len, GcmFrame &f) {
    f = GcmFrame{};
    if (iv_len != 12) return GCM_FMT_IV;
    if (!gcm_tag_len_ok(tag_len)) return GCM_FMT_TAG;
    f.tag_len = tag_len;
    f.aad_len = aad_len;
    f.data_len = data_len;
    const size_t n_blk = (data_len + 15) / 16, a_blk = (aad_len + 15) / 16;
    f.pub.assign((2 + n_blk) * 16, 0);
    for (size_t i = 0; i <= n_blk; i++) {
        uint8_t *b = &f.pub[(1 + i) * 16];
        std::memcpy(b, iv, 12);
        const uint32_t c = (uint32_t)(1 + i);  // J0 = 1, payload block i - 1 = 2 + (i - 1), modulo 2^32
        for (int j = 0; j < 4; j++) b[12 + j] = (uint8_t)(c >> (24 - 8 * j));
    }
    f.hashed.assign((a_blk + n_blk + 1) * 16, 0);
    if (aad_len) std::memcpy(f.hashed.data(), aad, aad_len);
    if (data_len) std::memcpy(&f.hashed[a_blk * 16], data, data_len);
    uint8_t *len = &f.hashed[(a_blk + n_blk) * 16];
    for (int j = 0; j < 8; j++) {
        len[j] = (uint8_t)(((uint64_t)aad_len * 8) >> (56 - 8 * j));
        len[8 + j] = (uint8_t)(((uint64_t)data_len * 8) >> (56 - 8 * j));
    }
    return GCM_FMT_OK;
}

// Row r < 8 tag_len of a frame: the sources (k, i), as 128 (k - 1) + i into the power table, for which coefficient r
// of X_(m + 1 - k) x^i is 1; ascending (k, i)
inline void gcm_frame_rows(const GcmFrame &f, std::vector<std::vector<int32_t>> &rows) {
    rows.assign((size_t)8 * f.tag_len, {});
    const size_t m = f.m();
    GcmElem cols[128];
    for (size_t k = 1; k <= m; k++) {
        gcm_mul_cols(gcm_from_bytes(&f.hashed[(m - k) * 16]), cols);
        for (int i = 0; i < 128; i++)
            for (size_t r = 0; r < rows.size(); r++)
                if (gcm_coef(cols[i], (int)r)) rows[r].push_back((int32_t)(128 * (k - 1) + i));
    }
}

constexpr int kGcmFirstChunk = 55;  // next to the E(J0) bit at level 9: 9 + 55 = 64
constexpr int kGcmNextChunk = 64;
constexpr int kGcmMaxChunks = 64;   // a tag-difference bit is the sum of its refreshed chunks

// chunks of a row of n level-1 sources: the first also takes the E(J0) bit
inline size_t gcm_row_chunks(size_t n) {
    return n <= (size_t)kGcmFirstChunk ? 1 : 1 + (n - kGcmFirstChunk + kGcmNextChunk - 1) / kGcmNextChunk;
}

enum GcmPlanStatus { GCM_PLAN_OK = 0, GCM_PLAN_POWERS, GCM_PLAN_NOISE };

// m <= n_powers, and no row beyond the two-level chunk sum
inline GcmPlanStatus gcm_frame_check(const GcmFrame &f, size_t n_powers,
                                     const std::vector<std::vector<int32_t>> &rows) {
    if (f.m() > n_powers) return GCM_PLAN_POWERS;
    for (const auto &r : rows)
        if (gcm_row_chunks(r.size()) > (size_t)kGcmMaxChunks) return GCM_PLAN_NOISE;
    return GCM_PLAN_OK;
}

// The plans of a call.  Source array of `chunks`: the power table's first table_blocks blocks, then E(J0) of every
// frame, [table_blocks + n_frames][128].  `diff` sums a row's refreshed chunks and adds the received tag bit.
struct GcmCallPlan {
    RowPlan chunks, diff;
    std::vector<int32_t> chunks_of_row;  // [n_frames * 8 tag_len]
};

inline void gcm_call_plan_add(GcmCallPlan &P, const std::vector<std::vector<int32_t>> &rows, size_t table_blocks,
                              size_t frame, const uint8_t *tag) {
    for (size_t r = 0; r < rows.size(); r++) {
        const std::vector<int32_t> &row = rows[r];
        int32_t n_chunks = 0;
        P.chunks.src.push_back((int32_t)((table_blocks + frame) * 128 + r));
        size_t room = kGcmFirstChunk;
        for (int32_t s : row) {
            if (!room) {
                P.chunks.end_row();
                P.diff.src.push_back((int32_t)P.chunks.n_rows() - 1);
                n_chunks++;
                room = kGcmNextChunk;
            }
            P.chunks.src.push_back(s);
            room--;
        }
        P.chunks.end_row();
        P.diff.src.push_back((int32_t)P.chunks.n_rows() - 1);
        n_chunks++;
        P.diff.end_row();
        P.diff.pub_bit.push_back((uint8_t)((tag[r >> 3] >> (7 - (r & 7))) & 1));
        P.chunks_of_row.push_back(n_chunks);
    }
}

// ---- segmented GHASH: frames beyond one table ----
// With e = m + 1 - i the exponent of X_i, c = (e - 1) / seg and k = (e - 1) % seg + 1:
//   GHASH = S_0 + sum_{c >= 1} S_c G_c,   S_c = sum_k X_(c,k) H^k,   G_c = H^(seg c)
// Every S_c is row sums over the table's first seg powers; an inner segment (c >= 1) is refreshed to a table-like
// element and lifted by one product with the stride power G_c (the stride key: H^(seg j) at entry j - 1, made by
// gcm_power_schedule on the base G_1).  C = ceil(m / seg) segments, C - 1 products.
//
// A hashed block puts at most 128 sources into a row, so an inner row holds at most 128 seg sources in chunks of 64
// and a final row 128 seg + (C - 1) <= 128 seg + 64 in chunks of 55 / 64.  For seg <= 31 that is at most
// 31 * 128 + 64 = 4032 <= 55 + 63 * 64 = 4087: no frame is refused for noise.  Beyond 31 it depends on the data.
constexpr int kGcmMaxStrides = 64;
constexpr int kGcmInnerChunk = 64;  // level-1 table bits per refreshed chunk of an inner row

inline size_t gcm_long_segments(size_t m, size_t seg) { return (m + seg - 1) / seg; }

// Segment c of a frame, rows r < n_rows: the sources (k, i), as 128 (k - 1) + i into the power table, for which
// coefficient r of X_(c,k) x^i is 1; ascending (k, i).  X_(c,k) is the hashed block of exponent seg c + k.  Segment 0
// with seg >= m is gcm_frame_rows.
inline void gcm_segment_rows(const GcmFrame &f, size_t seg, size_t c, size_t n_rows,
                             std::vector<std::vector<int32_t>> &rows) {
    rows.assign(n_rows, {});
    const size_t m = f.m(), kc = m - seg * c < seg ? m - seg * c : seg;
    GcmElem cols[128];
    for (size_t k = 1; k <= kc; k++) {
        gcm_mul_cols(gcm_from_bytes(&f.hashed[(m - (seg * c + k)) * 16]), cols);
        for (int i = 0; i < 128; i++)
            for (size_t r = 0; r < n_rows; r++)
                if (gcm_coef(cols[i], (int)r)) rows[r].push_back((int32_t)(128 * (k - 1) + i));
    }
}

// chunks of an inner row of n sources: no E(J0) bit; a row without a source is one empty chunk, the zero ciphertext
inline size_t gcm_inner_chunks(size_t n) { return n ? (n + kGcmInnerChunk - 1) / kGcmInnerChunk : 1; }

// The plans of a batch of inner segments.  `chunks` reads the power table's first seg blocks; `rows` sums a row's
// refreshed chunks: segment j of the batch is output rows 128 j .. 128 j + 127, refreshed once more into S_c.
struct GcmInnerPlan {
    RowPlan chunks, rows;
    std::vector<int32_t> chunks_of_row;  // [n_segments * 128]
};

inline void gcm_inner_plan_add(GcmInnerPlan &P, const std::vector<std::vector<int32_t>> &rows) {
    for (const std::vector<int32_t> &row : rows) {
        const size_t n_chunks = gcm_inner_chunks(row.size());
        for (size_t q = 0; q < n_chunks; q++) {
            const size_t a = q * kGcmInnerChunk, b = a + kGcmInnerChunk < row.size() ? a + kGcmInnerChunk : row.size();
            P.chunks.src.insert(P.chunks.src.end(), row.begin() + (std::ptrdiff_t)a, row.begin() + (std::ptrdiff_t)b);
            P.chunks.end_row();
            P.rows.src.push_back((int32_t)P.chunks.n_rows() - 1);
        }
        P.rows.end_row();
        P.chunks_of_row.push_back((int32_t)n_chunks);
    }
}

// The final rows of a frame: segment 0's sources, then bit r of every product S_c G_c, c ascending; product c - 1 of
// the frame is block first_product_block + c - 1 of the final source array.  Level-1 sources like any other.
inline void gcm_long_final_rows(const GcmFrame &f, size_t seg, size_t first_product_block,
                                std::vector<std::vector<int32_t>> &rows) {
    gcm_segment_rows(f, seg, 0, (size_t)8 * f.tag_len, rows);
    const size_t C = gcm_long_segments(f.m(), seg);
    for (size_t r = 0; r < rows.size(); r++)
        for (size_t c = 1; c < C; c++) rows[r].push_back((int32_t)((first_product_block + c - 1) * 128 + r));
}

enum GcmLongStatus { GCM_LONG_OK = 0, GCM_LONG_SEG, GCM_LONG_STRIDES, GCM_LONG_NOISE };

// seg in 1 .. min(n_powers, 64) (so the table holds min(seg, m) powers; ghash_key makes at most 64, and a caller's
// n_powers bounds nothing by itself), n_strides in 1 .. 64 and at least C - 1
inline GcmLongStatus gcm_long_shape_check(size_t m, size_t seg, size_t n_powers, size_t n_strides) {
    if (seg < 1 || seg > n_powers || seg > (size_t)kGcmMaxPowers) return GCM_LONG_SEG;
    if (n_strides < 1 || n_strides > (size_t)kGcmMaxStrides || gcm_long_segments(m, seg) - 1 > n_strides)
        return GCM_LONG_STRIDES;
    return GCM_LONG_OK;
}

inline bool gcm_inner_rows_ok(const std::vector<std::vector<int32_t>> &rows) {
    for (const auto &r : rows)
        if (gcm_inner_chunks(r.size()) > (size_t)kGcmMaxChunks) return false;
    return true;
}

inline bool gcm_final_rows_ok(const std::vector<std::vector<int32_t>> &rows) {
    for (const auto &r : rows)
        if (gcm_row_chunks(r.size()) > (size_t)kGcmMaxChunks) return false;
    return true;
}

// Every row of a frame, before any device work.  The shape comes first: rows are not walked for a refused shape.
inline GcmLongStatus gcm_long_frame_check(const GcmFrame &f, size_t seg, size_t n_powers, size_t n_strides) {
    const GcmLongStatus st = gcm_long_shape_check(f.m(), seg, n_powers, n_strides);
    if (st != GCM_LONG_OK) return st;
    std::vector<std::vector<int32_t>> rows;
    const size_t C = gcm_long_segments(f.m(), seg);
    for (size_t c = 1; c < C; c++) {
        gcm_segment_rows(f, seg, c, 128, rows);
        if (!gcm_inner_rows_ok(rows)) return GCM_LONG_NOISE;
    }
    gcm_long_final_rows(f, seg, 0, rows);
    return gcm_final_rows_ok(rows) ? GCM_LONG_OK : GCM_LONG_NOISE;
}

// ---- frames over key tables ----
// The chunk sums of a call read two source arrays (rowsum2_word): A, the power tables [n_keys][n_powers][128] where
// the caller keeps them, and B, E(J0) of every frame [n_frames][128].  A frame under slot s has the rows of the
// single-key call under the base 128 s n_powers, which selects the slot's table; its E(J0) entry is written relative
// to that base, so base + entry = |A| + 128 frame + r whatever the slot.  The sets summed are the single-key call's.
// A single key is the table of one slot: E(J0) of frame f at (n_powers + f) 128 + r.
enum GcmMultiStatus { GCM_MULTI_OK = 0, GCM_MULTI_SLOT, GCM_MULTI_TAG, GCM_MULTI_POWERS, GCM_MULTI_NOISE, GCM_MULTI_SIZE };

// what the plans of a call need, whatever its door: n_keys n_powers table blocks and a block per frame of 128 sources
// each, every index an int32_t
inline bool gcm_plan_index_ok(size_t n_keys, size_t n_powers, size_t n_frames) {
    const size_t cap = (size_t)1 << 24;
    return n_keys < cap && n_powers < cap && n_frames < cap && n_keys * n_powers + n_frames < cap;
}

// the key-table entry points and the key schedules refuse more: tables of at most 64 powers
inline bool gcm_multi_shape_ok(size_t n_keys, size_t n_powers, size_t n_frames) {
    return n_powers >= 1 && n_powers <= (size_t)kGcmMaxPowers && n_keys <= ((size_t)1 << 16) &&
           n_frames <= ((size_t)1 << 20);  // (2^16 * 64 + 2^20) * 128 < 2^31
}

// One frame of a call, before any device work: its slot, the call's tag length, then gcm_frame_check on its rows
inline GcmMultiStatus gcm_multi_frame_check(const GcmFrame &f, int64_t slot, size_t n_keys, size_t n_powers, int tag_len,
                                            const std::vector<std::vector<int32_t>> &rows) {
    if (slot < 0 || (uint64_t)slot >= n_keys) return GCM_MULTI_SLOT;
    if (f.tag_len != tag_len) return GCM_MULTI_TAG;
    switch (gcm_frame_check(f, n_powers, rows)) {
        case GCM_PLAN_POWERS: return GCM_MULTI_POWERS;
        case GCM_PLAN_NOISE: return GCM_MULTI_NOISE;
        default: return GCM_MULTI_OK;
    }
}

// gcm_call_plan_add for frame `frame` under slot `slot`: the same lists, E(J0) at |A| - base + 128 frame + r, and the
// slot's base on every chunk row the frame adds
inline void gcm_multi_plan_add(GcmCallPlan &P, const std::vector<std::vector<int32_t>> &rows, size_t n_keys,
                               size_t n_powers, size_t slot, size_t frame, const uint8_t *tag) {
    gcm_call_plan_add(P, rows, (n_keys - slot) * n_powers, frame, tag);
    P.chunks.base_of.resize(P.chunks.n_lists(), (int32_t)(slot * n_powers * 128));
}

}  // namespace tae
