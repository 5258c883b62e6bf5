// AEAD open under FHE: the tag verdict bit and the verdict-gated payload.  Plain C++ in the style of
// aes_ccm.hpp and aes_gcm.hpp: the plans and the truth tables have no device code, so a stand-alone program runs both
// plans on plain bits (tests/native/aead_open_test.cpp).
//
// The mode layer (CCM, multi-key CCM, GCM, segmented GCM) ends with the payload bits [sum len][8] of its frames, in
// order, and 8 tag_len tag-difference bits per frame that are all zero iff the frame is authentic.
//
//   verdict:  level 0 = the frame's 8 tag_len difference bits; every level groups its bits in eights, in order, the
//             last group padded with the zero ciphertext, and bootstraps each group through "OR of 8" (the last level,
//             one group: "NOR of 8").  ok = 1 iff every difference bit is 0.
//   gate:     payload byte g and the verdict bit of its frame through one 9 -> 8 table, out_i = in_i AND in_8: the
//             plaintext when the tag is right, all zeros when it is not.
//
// N = 512 takes nine table inputs with no CMux tree (vertical_packing, n_in <= log2 N).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tae {

constexpr int kOpenOrBits = 8;    // inputs of a verdict group
constexpr int kOpenGateBits = 9;  // inputs of a gate group: the byte's 8 bits, then the verdict bit
constexpr int kOpenGateBlockBytes = 14;  // gate groups per cipher block's worth of scratch: 9 * 14 = 126 <= 128 bits

// the tag lengths CCM (4 .. 16, even) and GCM (4, 8, 12 .. 16) accept
inline bool aead_tag_len_ok(int tag_len) {
    const bool ccm = tag_len >= 4 && tag_len <= 16 && !(tag_len & 1);
    const bool gcm = tag_len == 4 || tag_len == 8 || (tag_len >= 12 && tag_len <= 16);
    return ccm || gcm;
}

// ---- the truth tables, as value arrays for generate_lookup_table: v holds the group's inputs MSB first, the value
// holds output j at bit n_out - 1 - j ----
inline uint64_t aead_or8(unsigned v) { return (v & 0xFF) ? 1 : 0; }
inline uint64_t aead_nor8(unsigned v) { return (v & 0xFF) ? 0 : 1; }
// v = the byte's 8 bits (bits 8 .. 1 of v), then the verdict (bit 0)
inline uint64_t aead_gate9(unsigned v) { return (v & 1) ? (v >> 1) & 0xFF : 0; }

struct AeadOpenTables {
    std::vector<uint64_t> or8, nor8, gate;  // [256], [256], [512]
};

inline AeadOpenTables aead_open_tables() {
    AeadOpenTables t;
    t.or8.resize(256), t.nor8.resize(256), t.gate.resize(512);
    for (unsigned v = 0; v < 256; v++) t.or8[v] = aead_or8(v), t.nor8[v] = aead_nor8(v);
    for (unsigned v = 0; v < 512; v++) t.gate[v] = aead_gate9(v);
    return t;
}

// ---- the verdict plan.  Level l has bits[l] bits per frame (bits[0] = 8 tag_len) in groups[l] = ceil(bits[l] / 8)
// groups; bits[l + 1] = groups[l]; the last level has one group.  idx[l] [n_frames][groups[l]][8] indexes the level's
// small ciphertexts [n_frames][bits[l]], -1 the zero ciphertext ----
struct VerdictPlan {
    size_t n_frames = 0;
    std::vector<size_t> bits, groups;
    std::vector<std::vector<int32_t>> idx;
    int levels() const { return (int)groups.size(); }
};

inline VerdictPlan aead_verdict_plan(int tag_len, size_t n_frames) {
    VerdictPlan p;
    p.n_frames = n_frames;
    for (size_t b = 8 * (size_t)tag_len;; b = p.groups.back()) {
        const size_t G = (b + kOpenOrBits - 1) / kOpenOrBits;
        p.bits.push_back(b);
        p.groups.push_back(G);
        std::vector<int32_t> ix(n_frames * G * kOpenOrBits);
        for (size_t f = 0; f < n_frames; f++)
            for (size_t s = 0; s < G * kOpenOrBits; s++)
                ix[f * G * kOpenOrBits + s] = s < b ? (int32_t)(f * b + s) : -1;
        p.idx.push_back(std::move(ix));
        if (G == 1) break;
    }
    return p;
}

// ---- the gate plan.  Byte g (frames in order) is in frame frame_of_byte[g]; a frame of length 0 has no group ----
struct GatePlan {
    size_t n_frames = 0;
    std::vector<int32_t> frame_of_byte;  // [sum payload_lens]
    size_t n_bytes() const { return frame_of_byte.size(); }
};

inline GatePlan aead_gate_plan(const size_t *payload_lens, size_t n_frames) {
    GatePlan p;
    p.n_frames = n_frames;
    for (size_t f = 0; f < n_frames; f++) p.frame_of_byte.insert(p.frame_of_byte.end(), payload_lens[f], (int32_t)f);
    return p;
}

// The index table of the gate groups of bytes g0 .. g0 + n - 1 [n][9] into the small ciphertexts of one pass: the
// n_frames verdict bits first, then the pass's payload bits [n][8]
inline std::vector<int32_t> aead_gate_pass_index(const GatePlan &p, size_t g0, size_t n) {
    std::vector<int32_t> ix(n * kOpenGateBits);
    for (size_t g = 0; g < n; g++) {
        for (int b = 0; b < 8; b++) ix[g * kOpenGateBits + b] = (int32_t)(p.n_frames + g * 8 + b);
        ix[g * kOpenGateBits + 8] = p.frame_of_byte[g0 + g];
    }
    return ix;
}

// ---- both plans on plain bits: what the device computes, for the tests ----
// diff [n_frames][8 tag_len] -> ok [n_frames]
inline std::vector<uint8_t> aead_verdict_plain(const VerdictPlan &p, std::vector<uint8_t> cur) {
    for (int l = 0; l < p.levels(); l++) {
        const bool last = l + 1 == p.levels();
        std::vector<uint8_t> next(p.n_frames * p.groups[l]);
        for (size_t t = 0; t < next.size(); t++) {
            unsigned v = 0;
            for (int b = 0; b < kOpenOrBits; b++) {
                const int32_t s = p.idx[l][t * kOpenOrBits + b];
                v = (v << 1) | (s < 0 ? 0u : (unsigned)(cur[(size_t)s] & 1));
            }
            next[t] = (uint8_t)(last ? aead_nor8(v) : aead_or8(v));
        }
        cur.swap(next);
    }
    return cur;
}

// plain [n_bytes][8] (MSB first), ok [n_frames] -> gated [n_bytes][8], in passes of `pass` bytes
inline std::vector<uint8_t> aead_gate_plain(const GatePlan &p, const std::vector<uint8_t> &plain,
                                            const std::vector<uint8_t> &ok, size_t pass) {
    std::vector<uint8_t> out(plain.size());
    for (size_t g0 = 0; g0 < p.n_bytes(); g0 += pass) {
        const size_t n = p.n_bytes() - g0 < pass ? p.n_bytes() - g0 : pass;
        std::vector<uint8_t> small(ok);
        small.insert(small.end(), plain.begin() + (std::ptrdiff_t)(g0 * 8), plain.begin() + (std::ptrdiff_t)((g0 + n) * 8));
        const std::vector<int32_t> ix = aead_gate_pass_index(p, g0, n);
        for (size_t g = 0; g < n; g++) {
            unsigned v = 0;
            for (int b = 0; b < kOpenGateBits; b++) v = (v << 1) | (unsigned)(small[(size_t)ix[g * kOpenGateBits + b]] & 1);
            const uint64_t r = aead_gate9(v);
            for (int j = 0; j < 8; j++) out[(g0 + g) * 8 + j] = (uint8_t)((r >> (7 - j)) & 1);
        }
    }
    return out;
}

}  // namespace tae
