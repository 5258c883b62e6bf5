// Host-side model mirror: noise bookkeeping, circuit_bootstrap, AES round driver, key schedule.
// See model.hpp for the reference mapping.
#include "model.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <deque>

#include "aes.hpp"
#include "aes_inv.hpp"
#include "aes_xts.hpp"
#include "cplx.hpp"
#include "glwe_pack.hpp"
#include "../../include/tfhe_aes_gpu.h"

namespace tae {

void gf_256_mul_bit_terms(uint8_t b, int terms[8][8]) {
    int a[8][8] = {}, res[8][8] = {};
    for (int i = 0; i < 8; i++) a[i][i] = 1;
    for (int it = 0; it < 8; it++) {
        if (b & 1)
            for (int o = 0; o < 8; o++)
                for (int i = 0; i < 8; i++) res[o][i] += a[o][i];
        // Byte::shl_assign_1 (data_model.rs:45-49): bit 0 leaves, the rest rotate left, a trivial
        // zero enters at bit 7; the leaving bit is XORed into bits 3, 4, 6, 7
        int red[8];
        for (int i = 0; i < 8; i++) red[i] = a[0][i];
        for (int o = 0; o < 7; o++)
            for (int i = 0; i < 8; i++) a[o][i] = a[o + 1][i];
        for (int i = 0; i < 8; i++) a[7][i] = 0;
        for (int tap : {3, 4, 6, 7})
            for (int i = 0; i < 8; i++) a[tap][i] += red[i];
        b >>= 1;
    }
    for (int o = 0; o < 8; o++)
        for (int i = 0; i < 8; i++) terms[o][i] = res[o][i];
}

void mix_column_terms(int terms[32][32]) {
    int g[4][8][8];
    for (int m = 1; m <= 3; m++) gf_256_mul_bit_terms((uint8_t)m, g[m]);
    for (int o = 0; o < 32; o++)
        for (int i = 0; i < 32; i++) terms[o][i] = 0;
    for (int r = 0; r < 4; r++)
        for (int o = 0; o < 8; o++)
            for (int x = 0; x < 8; x++) {
                terms[8 * r + o][8 * r + x] += g[2][o][x];
                terms[8 * r + o][8 * ((r + 3) % 4) + x] += g[1][o][x];
                terms[8 * r + o][8 * ((r + 2) % 4) + x] += g[1][o][x];
                terms[8 * r + o][8 * ((r + 1) % 4) + x] += g[3][o][x];
            }
}

// ---------------------------------------------------------------------------------------------
// Noise bookkeeping
// ---------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_ct_counter{0};
uint64_t next_ct_id() { return g_ct_counter.fetch_add(1); }

void NoiseLevel::add_assign(const NoiseLevel &rhs, uint64_t max_noise_sq) {
    // assert!(components ∩ rhs.components == ∅, "noise components not independent")
    auto a = components.cbegin();
    auto b = rhs.components.cbegin();
    while (a != components.cend() && b != rhs.components.cend()) {
        if (*a == *b) throw ModelError{TAE_E_INDEP, "noise components not independent"};
        if (*a < *b)
            ++a;
        else
            ++b;
    }
    std::vector<uint64_t> merged;
    merged.reserve(components.size() + rhs.components.size());
    std::merge(components.begin(), components.end(), rhs.components.begin(), rhs.components.end(),
               std::back_inserter(merged));
    components.swap(merged);
    noise_level_squared += rhs.noise_level_squared;
    if (noise_level_squared > max_noise_sq)  // MaxNoiseLevel::validate(..).unwrap()
        throw ModelError{TAE_E_NOISE, "NoiseTooBig { noise_level: " + std::to_string(noise_level_squared) +
                                          ", max_noise_level: " + std::to_string(max_noise_sq) + " }"};
}

void BitCt::xor_assign(const BitCt &rhs) {
    if (rhs.ct.size() != ct.size()) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
    for (size_t i = 0; i < ct.size(); i++) ct[i] += rhs.ct[i];  // lwe_ciphertext_add_assign
    noise.add_assign(rhs.noise, max_noise_sq);
}

BitCt Context::trivial(uint64_t bit) const {
    if (bit > 1) throw ModelError{TAE_E_ARG, "cleartext out of bounds: " + std::to_string(bit)};
    BitCt b;
    b.ct.assign(bit_len(), 0);
    b.ct.back() = params().model == 2 ? bit << 62 : encode_bit(bit);  // shortint create_trivial: m * delta
    b.noise = NoiseLevel::trivial();
    b.max_noise_sq = params().max_noise_sq;
    return b;
}

BitCt Context::wrap(std::vector<uint64_t> ct, uint64_t noise_level_squared) const {
    BitCt b;
    b.ct = std::move(ct);
    // 8-bit model: shortint NoiseLevel (additive, no component ids; shortint_woppbs_8bit.rs:94-163);
    // shortint_1bit: XOR is unchecked_add (shortint_1bit.rs:103-116), nothing is tracked
    b.noise = params().model == 8   ? NoiseLevel{noise_level_squared, {}}
              : params().model == 2 ? NoiseLevel{}
                                    : NoiseLevel::with_noise_level(noise_level_squared, next_ct_id());
    b.max_noise_sq = params().max_noise_sq;
    return b;
}

Lut Context::generate_lookup_table(int input_bits, int output_bits, const uint64_t *f_values) const {
    if (!(input_bits > 0 && input_bits <= 16)) throw ModelError{TAE_E_PARAM, "input_bits must be in 1..=16"};
    if (!(output_bits > 0 && output_bits <= 64)) throw ModelError{TAE_E_PARAM, "output_bits must be in 1..=64"};
    Lut l;
    l.input_bits = input_bits;
    l.output_bits = output_bits;
    if (params().model == 8) {
        // 8-bit model: FheContext::generate_lookup_table (shortint_woppbs_8bit.rs:262-265) is a byte ->
        // byte map through WopbsKey::generate_lut_without_padding (one polynomial, 2^56 scale)
        if (input_bits != 8 || output_bits != 8)
            throw ModelError{TAE_E_PARAM, "the 8-bit model's lookup tables map 8 bits to 8 bits"};
        l.small_len = (size_t)std::max(params().N, 256);
        l.data.assign(l.small_len, 0);
        generate_lut_without_padding(params().N, f_values, l.data.data());
        return l;
    }
    l.small_len = lut_small_len(params().N, input_bits);
    l.data.assign(l.small_len * output_bits, 0);
    generate_lut(params().N, input_bits, output_bits, f_values, l.data.data());
    return l;
}

// The staging scope of one entry point: it holds the context's lock, sets its device and hands the engine the arrays
// of the call.  Device memory (TAE_MEM_DEVICE) passes through, ordered after the caller's work; host memory is
// uploaded into buffers the scope owns (one hipMalloc per array) and the outputs are downloaded by finish().  The
// destructor only frees: an exception before finish() leaves the caller's outputs untouched.
class Context::Staged {
  public:
    Staged(Context &c, bool device_mem) : lock_(c.mu_), e_(*c.engine_), dev_(device_mem) {
        hip_check(hipSetDevice(e_.device()), "hipSetDevice");
        if (dev_) e_.order_after_caller();
    }
    // n elements the engine reads: the caller's array, or its upload
    template <class T>
    const T *in(const T *p, size_t n) {
        return dev_ ? p : upload(p, n);
    }
    // public bytes, lookup tables, test vectors: host arrays, always; null or empty stays null
    template <class T>
    const T *pub(const T *p, size_t n) {
        return p && n ? upload(p, n) : nullptr;
    }
    // n elements the engine writes: the caller's array, or a buffer that finish() downloads into it
    template <class T>
    T *out(T *p, size_t n) {
        if (dev_) return p;
        T *d = alloc<T>(n);
        downloads_.push_back({p, d, n * sizeof(T)});
        return d;
    }
    // ... for a stage that does not write every word: the host caller reads zeros there (a device array is the
    // caller's to clear)
    template <class T>
    T *out_zeroed(T *p, size_t n) {
        T *d = out(p, n);
        if (!dev_ && n) hip_check(hipMemsetAsync(d, 0, n * sizeof(T), e_.stream()), "clear output");
        return d;
    }
    // n elements the engine updates in place: the caller's array, or its upload, downloaded by finish()
    template <class T>
    T *inout(T *p, size_t n) {
        if (dev_) return p;
        T *d = const_cast<T *>(upload(p, n));
        downloads_.push_back({p, d, n * sizeof(T)});
        return d;
    }
    // a lookup table or test vector in the memory kind of the call
    template <class T>
    const T *lut(const T *p, size_t n) {
        return dev_ ? p : pub(p, n);
    }
    // a key table [..][stride]: the caller's, or a compact upload of only the slots that `slots` refers to, which is
    // rewritten to index it, so a slot that nothing refers to is not read in either case
    const uint64_t *table(const uint64_t *table, std::vector<int32_t> &slots, size_t stride);
    // a call outside the engine's AES and mode drivers (Engine::begin_call): the stage times restart here, after
    // the call's own checks, and finish() sums what it recorded
    void own_times() {
        e_.begin_call();
        own_times_ = true;
    }
    // the downloads, in the order of their out() calls, then the engine's synchronize
    void finish() {
        if (own_times_) e_.end_call();
        for (const Download &d : downloads_)
            if (d.bytes) hip_check(hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, e_.stream()), "download");
        e_.synchronize();
    }

  private:
    struct Download {
        void *host;
        const void *dev;
        size_t bytes;
    };
    template <class T>
    T *alloc(size_t n) {
        bufs_.emplace_back(n * sizeof(T));
        return reinterpret_cast<T *>(bufs_.back().get());
    }
    template <class T>
    const T *upload(const T *p, size_t n) {
        T *d = alloc<T>(n);
        if (n) hip_check(hipMemcpyAsync(d, p, n * sizeof(T), hipMemcpyHostToDevice, e_.stream()), "upload");
        return d;
    }
    std::lock_guard<std::mutex> lock_;
    Engine &e_;
    const bool dev_;
    bool own_times_ = false;
    std::deque<DevBuf<uint8_t>> bufs_;  // freed before the lock is released
    std::vector<Download> downloads_;
};

// words [n][L] as n bits carrying noise[i]
static std::vector<BitCt> wrap_bits(const std::vector<uint64_t> &words, std::vector<NoiseLevel> noise, size_t L,
                                    uint64_t max_noise_sq) {
    std::vector<BitCt> bits(noise.size());
    for (size_t i = 0; i < bits.size(); i++) {
        bits[i].ct.assign(words.begin() + i * L, words.begin() + (i + 1) * L);
        bits[i].noise = std::move(noise[i]);
        bits[i].max_noise_sq = max_noise_sq;
    }
    return bits;
}

// the levels of whole blocks [n][128] as one list, cut to n_bits
static std::vector<NoiseLevel> flat_noise(std::vector<std::vector<NoiseLevel>> blocks, size_t n_bits) {
    std::vector<NoiseLevel> flat;
    flat.reserve(blocks.size() * 128);
    for (auto &b : blocks)
        for (NoiseLevel &x : b) flat.push_back(std::move(x));
    flat.resize(n_bits);
    return flat;
}

void Context::bootstrap_from_bits_raw(const uint64_t *bits, size_t groups, const Lut &lut, uint64_t *out,
                                      bool device_mem) {
    if (params().model != 8) throw ModelError{TAE_E_PARAM, "bootstrap_from_bits belongs to the 8-bit model"};
    if (lut.input_bits != 8) throw ModelError{TAE_E_ARG, "bootstrap_from_bits needs an 8-bit LUT"};
    Staged st(*this, device_mem);
    st.own_times();
    engine_->cbs_vp(st.in(bits, groups * 8 * bit_len()), groups, 8, st.pub(lut.data.data(), lut.data.size()), 1,
                    st.out(out, groups * params().big_len()));
    st.finish();
}

void Context::extract_bits_raw(const uint64_t *ints, size_t groups, uint64_t *out, bool device_mem) {
    if (params().model != 8) throw ModelError{TAE_E_PARAM, "extract_bits_from_ciphertext belongs to the 8-bit model"};
    Staged st(*this, device_mem);
    st.own_times();
    engine_->extract_bits(st.in(ints, groups * params().big_len()), groups, 56, 8, st.out(out, groups * 8 * bit_len()));
    st.finish();
}

void Context::circuit_bootstrap_raw(const uint64_t *bits, size_t groups, int n_in, const Lut &lut, uint64_t *out,
                                    bool device_mem) {
    if (n_in != lut.input_bits) throw ModelError{TAE_E_ARG, "number of input bits does not match the LUT"};
    Staged st(*this, device_mem);
    st.own_times();
    const uint64_t *d_lut = st.pub(lut.data.data(), lut.data.size());
    if (params().model == 8) {
        // Byte::bootstrap_with_lut (fhe_impls/shortint_woppbs_8bit.rs:37-42): bits [G][8][n+1] -> [G][8][n+1]
        const size_t len = groups * 8 * bit_len();
        engine_->bootstrap_bytes8(st.in(bits, len), groups, d_lut, st.out(out, len));
    } else {
        const size_t L = params().big_len();
        engine_->circuit_bootstrap(st.in(bits, groups * n_in * L), groups, n_in, d_lut, lut.output_bits,
                                   st.out(out, groups * lut.output_bits * L));
    }
    st.finish();
}

// FheContext::circuit_bootstrap (shortint_woppbs_1bit.rs:292-336)
std::vector<BitCt> Context::circuit_bootstrap(const std::vector<const BitCt *> &bits, const Lut &lut) {
    const size_t L = bit_len();
    for (const BitCt *b : bits)
        if (b->ct.size() != L) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
    if (params().model == 8) {
        // Byte::bootstrap_with_lut: extract_bits outputs are BitCt::new (NOMINAL noise)
        if (bits.size() != 8) throw ModelError{TAE_E_ARG, "the 8-bit model bootstraps whole bytes"};
        std::vector<uint64_t> in8(8 * L), out8(8 * L);
        for (size_t b = 0; b < 8; b++) std::memcpy(&in8[b * L], bits[b]->ct.data(), L * 8);
        circuit_bootstrap_raw(in8.data(), 1, 8, lut, out8.data(), false);
        std::vector<BitCt> res;
        for (int j = 0; j < 8; j++)
            res.push_back(wrap(std::vector<uint64_t>(out8.begin() + j * L, out8.begin() + (j + 1) * L), 1));
        return res;
    }
    std::vector<uint64_t> in(bits.size() * L), out((size_t)lut.output_bits * L);
    for (size_t b = 0; b < bits.size(); b++) std::memcpy(&in[b * L], bits[b]->ct.data(), L * 8);
    circuit_bootstrap_raw(in.data(), 1, (int)bits.size(), lut, out.data(), false);
    // Lemma 3.2 of eprint 2017/430: output noise^2 = NOMINAL * input_bit_count (:322-325)
    std::vector<BitCt> res;
    for (int j = 0; j < lut.output_bits; j++)
        res.push_back(wrap(std::vector<uint64_t>(out.begin() + j * L, out.begin() + (j + 1) * L), bits.size()));
    return res;
}

// ---------------------------------------------------------------------------------------------
// AES (fhe_sbox_gal_mul_pbs.rs)
// ---------------------------------------------------------------------------------------------
// Metadata-only replay of encrypt_block_for_rounds for ONE block: rk [4 (nr + 1) * 32], block [128].
// The rounds after round 0: st [128] is the state with round key 0 added.  last_key == false leaves the last round
// key out: the last SubBytes output after ShiftRows alone (CCM's X').
static std::vector<NoiseLevel> aes_noise_rounds(const std::vector<NoiseLevel> &rk, std::vector<NoiseLevel> st, int rounds,
                                                uint64_t max, int nr, bool last_key);

std::vector<NoiseLevel> aes_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &block,
                                           int rounds, uint64_t max, int nr) {
    std::vector<NoiseLevel> st = block;  // index (4*col + row)*8 + bit
    for (int i = 0; i < 128; i++) st[i].add_assign(rk[i], max);  // round key 0: words 0..3, the state's order
    return aes_noise_rounds(rk, std::move(st), rounds, max, nr, true);
}

static std::vector<NoiseLevel> aes_noise_rounds(const std::vector<NoiseLevel> &rk, std::vector<NoiseLevel> st, int rounds,
                                                uint64_t max, int nr, bool last_key) {
    auto key_bit = [&](int word, int byte, int bit) -> const NoiseLevel & { return rk[(word * 4 + byte) * 8 + bit]; };
    auto cbs_outputs = [&](int n_out) {
        std::vector<NoiseLevel> o((size_t)16 * n_out);
        for (auto &x : o) x = NoiseLevel::with_noise_level(8, next_ct_id());
        return o;
    };
    for (int round = 1; round < rounds; round++) {
        std::vector<NoiseLevel> muls = cbs_outputs(24);  // [byte][24]
        auto src = [&](int rr, int c, int m, int b) -> const NoiseLevel & {
            return muls[(4 * ((c + rr) % 4) + rr) * 24 + 8 * m + b];
        };
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++)
                for (int b = 0; b < 8; b++) {
                    NoiseLevel v = src(r, c, 1, b);
                    v.add_assign(src((r + 3) % 4, c, 0, b), max);
                    v.add_assign(src((r + 2) % 4, c, 0, b), max);
                    v.add_assign(src((r + 1) % 4, c, 2, b), max);
                    v.add_assign(key_bit(4 * round + c, r, b), max);
                    st[(4 * c + r) * 8 + b] = std::move(v);
                }
    }
    std::vector<NoiseLevel> sb = cbs_outputs(8);
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++)
            for (int b = 0; b < 8; b++) {
                NoiseLevel v = sb[(4 * ((c + r) % 4) + r) * 8 + b];
                if (last_key) v.add_assign(key_bit(4 * nr + c, r, b), max);
                st[(4 * c + r) * 8 + b] = std::move(v);
            }
    return st;
}

// fhe_sbox_pbs::encrypt_block_for_rounds (:75-121) on metadata: SubBytes = bootstrap_with_lut
// (outputs NOMINAL), MixColumns adds the network's terms, ARK the key bit.
std::vector<NoiseLevel> aes8_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &block,
                                            int rounds, uint64_t max) {
    int terms[32][32];
    mix_column_terms(terms);
    auto key_bit = [&](int word, int byte, int bit) -> const NoiseLevel & { return rk[(word * 4 + byte) * 8 + bit]; };
    std::vector<NoiseLevel> st = block;
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++)
            for (int b = 0; b < 8; b++) st[(4 * c + r) * 8 + b].add_assign(key_bit(c, r, b), max);
    const NoiseLevel nominal{1, {}};
    for (int round = 1; round <= rounds; round++) {
        const bool last = round == rounds;
        for (int c = 0; c < 4; c++)
            for (int o = 0; o < 32; o++) {
                NoiseLevel v{0, {}};
                if (last) {
                    v = nominal;
                } else {
                    for (int i = 0; i < 32; i++)
                        for (int t = 0; t < terms[o][i]; t++) v.add_assign(nominal, max);
                }
                v.add_assign(key_bit(last ? 40 + c : 4 * round + c, o / 8, o % 8), max);
                st[(4 * c + o / 8) * 8 + o % 8] = std::move(v);
            }
    }
    return st;
}

// fhe_sbox_pbs::gf_256_mul (:33-53) on the 1-bit model's noise metadata, XOR by XOR (MSB-first bits,
// Byte::shl_assign_1 = data_model.rs:45-49).  The loop keeps shifting and reducing the multiplicand
// after the last multiplier bit: from the fifth iteration on, the leaving bit already carries the
// component of the original bit 0 that the reduction XORs into bits 3, 4, 6, 7 again, so every call
// raises "noise components not independent" on non-trivial inputs.
static std::array<NoiseLevel, 8> gf_256_mul_noise(const std::array<NoiseLevel, 8> &x, uint8_t b, uint64_t max) {
    std::array<NoiseLevel, 8> a = x, res;  // res = Byte::trivial(ctx, 0)
    for (int it = 0; it < 8; it++) {
        if (b & 1)
            for (int i = 0; i < 8; i++) res[i].add_assign(a[i], max);
        const NoiseLevel reduce_x8 = a[0];
        for (int i = 0; i < 7; i++) a[i] = a[i + 1];
        a[7] = NoiseLevel::trivial();
        for (int tap : {3, 4, 6, 7}) a[tap].add_assign(reduce_x8, max);
        b >>= 1;
    }
    return res;
}

// fhe_sbox_pbs::encrypt_block_for_rounds (:75-121) over the 1-bit model (ShortintWoppbs1BitSboxPbsAesEncrypt,
// fhe_impls/shortint_woppbs_1bit.rs:47-81) on metadata: SubBytes = Byte::sbox_substitute (one 8 -> 8
// circuit bootstrap, outputs noise^2 = 8 with fresh ids), ShiftRows, MixColumns = the gf_256_mul network
// (:56-73), AddRoundKey.  MixColumns always raises TAE_E_INDEP (gf_256_mul_noise), which is why the
// reference #[ignore]s test_light / test_full of this combination (:160-176): only a 1-round run passes.
std::vector<NoiseLevel> sbox_pbs_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &block,
                                                int rounds, uint64_t max) {
    auto key_bit = [&](int word, int byte, int bit) -> const NoiseLevel & { return rk[(word * 4 + byte) * 8 + bit]; };
    std::vector<NoiseLevel> st = block;  // index (4*col + row)*8 + bit (State::from_array)
    auto xor_state = [&](int w0) {
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++)
                for (int b = 0; b < 8; b++) st[(4 * c + r) * 8 + b].add_assign(key_bit(w0 + c, r, b), max);
    };
    auto sub_bytes_shift_rows = [&] {
        std::vector<NoiseLevel> sb(128);
        for (auto &x : sb) x = NoiseLevel::with_noise_level(8, next_ct_id());
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++)
                for (int b = 0; b < 8; b++) st[(4 * c + r) * 8 + b] = sb[(4 * ((c + r) % 4) + r) * 8 + b];
    };
    xor_state(0);
    for (int round = 1; round < rounds; round++) {
        sub_bytes_shift_rows();
        std::vector<NoiseLevel> mixed(128);
        for (int c = 0; c < 4; c++) {
            std::array<NoiseLevel, 8> col[4];
            for (int r = 0; r < 4; r++)
                for (int b = 0; b < 8; b++) col[r][b] = st[(4 * c + r) * 8 + b];
            for (int i = 0; i < 4; i++) {
                std::array<NoiseLevel, 8> v = gf_256_mul_noise(col[i], 2, max);
                for (const auto &[src, m] : {std::pair<int, uint8_t>{(i + 3) % 4, 1}, {(i + 2) % 4, 1}, {(i + 1) % 4, 3}}) {
                    const std::array<NoiseLevel, 8> t = gf_256_mul_noise(col[src], m, max);
                    for (int b = 0; b < 8; b++) v[b].add_assign(t[b], max);
                }
                for (int b = 0; b < 8; b++) mixed[(4 * c + i) * 8 + b] = v[b];
            }
        }
        st.swap(mixed);
        xor_state(4 * round);
    }
    sub_bytes_shift_rows();
    xor_state(40);
    return st;
}

std::vector<NoiseLevel> Context::block_noise_schedule(AesDriver driver, const std::vector<NoiseLevel> &rk,
                                                      const std::vector<NoiseLevel> &block, int rounds, int nr) const {
    const uint64_t max = params().max_noise_sq;
    // shortint_1bit: XOR is shortint unchecked_add (shortint_1bit.rs:103-116) and SubBytes a fresh
    // bootstrap: nothing is validated, so the round function cannot fail on noise bookkeeping (its
    // decryption failures are the reference's #[ignore]d "too big noise accumulation")
    if (params().model == 2) return std::vector<NoiseLevel>(128);
    if (params().model == 8) return aes8_noise_schedule(rk, block, rounds, max);
    return driver == AesDriver::SboxPbs ? sbox_pbs_noise_schedule(rk, block, rounds, max)
                                        : aes_noise_schedule(rk, block, rounds, max, nr);
}

// key_bits in {128, 192, 256} or TAE_E_PARAM; 192 and 256 on the 1-bit model with the gal-mul driver only (the
// scope of the inverse cipher).  Returns Nr.
int Context::require_key_bits(int key_bits, AesDriver driver) const {
    if (!aes_key_bits_ok(key_bits)) throw ModelError{TAE_E_PARAM, "key_bits must be 128, 192 or 256"};
    if (key_bits != 128 && (params().model != 1 || driver != AesDriver::GalMul))
        throw ModelError{TAE_E_PARAM,
                         "AES-192 and AES-256 run on the 1-bit WoP-PBS parameter sets (gal-mul driver) only"};
    return aes_nr(key_bits);
}

static void require_rounds(int rounds, int nr) {
    if (rounds < 1 || rounds > nr) throw ModelError{TAE_E_PARAM, "rounds must be in 1..=" + std::to_string(nr)};
}

static void require_key_words(size_t bits, int nr, const char *what) {
    const int words = 4 * (nr + 1);
    if (bits != (size_t)words * 32)
        throw ModelError{TAE_E_ARG, std::string(what) + " must be " + std::to_string(words) + " words (" +
                                        std::to_string(words * 32) + " bits)"};
}

// The device round functions.  1-bit model: Engine::aes_encrypt_blocks (fhe_sbox_gal_mul_pbs rounds, its
// last round = SubBytes 8 -> 8, ShiftRows, AddRoundKey).  The 1-bit fhe_sbox_pbs driver only gets here
// with rounds == 1 (its schedule raises at the first MixColumns), where it is exactly that last round.
void Context::run_aes_blocks(AesDriver driver, const uint64_t *d_rk, const uint64_t *d_in, size_t n_blocks, int rounds,
                             uint64_t *d_out, int nr) {
    if (params().model == 8) {
        engine_->aes8_encrypt_blocks(d_rk, d_in, n_blocks, rounds, d_out);
        return;
    }
    if (params().model == 2) {
        engine_->s1_aes_encrypt_blocks(d_rk, d_in, n_blocks, rounds, d_out);
        return;
    }
    if (driver == AesDriver::SboxPbs && rounds != 1)
        throw ModelError{TAE_E_INDEP, "noise components not independent"};
    engine_->aes_encrypt_blocks(d_rk, d_in, n_blocks, rounds, d_out, nr);
}

void Context::aes_encrypt_blocks_raw(const uint64_t *rk, const uint64_t *blocks, size_t n_blocks, int rounds,
                                     uint64_t *out, bool device_mem, AesDriver driver, int key_bits) {
    const int nr = require_key_bits(key_bits, driver);
    const size_t kw = (size_t)aes_words(key_bits) * 32;  // ciphertexts of the expanded key
    require_rounds(rounds, nr);
    {
        // static validation of the fixed noise schedule for fresh inputs (noise^2 = 1, own ids)
        std::vector<NoiseLevel> krk(kw), kbl(128);
        for (auto &x : krk) x = params().model != 1 ? NoiseLevel{1, {}} : NoiseLevel::with_noise_level(1, next_ct_id());
        for (auto &x : kbl) x = params().model != 1 ? NoiseLevel{1, {}} : NoiseLevel::with_noise_level(1, next_ct_id());
        block_noise_schedule(driver, krk, kbl, rounds, nr);
    }
    const size_t S = bit_len(), len = n_blocks * 128 * S;
    Staged st(*this, device_mem);
    run_aes_blocks(driver, st.in(rk, kw * S), st.in(blocks, len), n_blocks, rounds, st.out(out, len), nr);
    st.finish();
}

std::vector<BitCt> Context::aes_encrypt_blocks(const std::vector<const BitCt *> &expanded_key,
                                               const std::vector<const BitCt *> &blocks, size_t n_blocks,
                                               int rounds, AesDriver driver, int key_bits) {
    const int nr = require_key_bits(key_bits, driver);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    require_key_words(expanded_key.size(), nr, "expanded key");
    if (blocks.size() != n_blocks * 128) throw ModelError{TAE_E_ARG, "blocks must be 128 bits each"};
    require_rounds(rounds, nr);
    const size_t L = bit_len();
    for (const BitCt *b : expanded_key)
        if (b->ct.size() != L) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
    for (const BitCt *b : blocks)
        if (b->ct.size() != L) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
    std::vector<NoiseLevel> krk(kw);
    for (size_t i = 0; i < krk.size(); i++) krk[i] = expanded_key[i]->noise;
    std::vector<std::vector<NoiseLevel>> out_noise(n_blocks);
    for (size_t blk = 0; blk < n_blocks; blk++) {
        std::vector<NoiseLevel> kb(128);
        for (int i = 0; i < 128; i++) kb[i] = blocks[blk * 128 + i]->noise;
        out_noise[blk] = block_noise_schedule(driver, krk, kb, rounds, nr);
    }
    std::vector<uint64_t> rk(kw * L), in(n_blocks * 128 * L), out(n_blocks * 128 * L);
    for (size_t i = 0; i < kw; i++) std::memcpy(&rk[i * L], expanded_key[i]->ct.data(), L * 8);
    for (size_t i = 0; i < n_blocks * 128; i++) std::memcpy(&in[i * L], blocks[i]->ct.data(), L * 8);
    {
        Staged st(*this, false);
        run_aes_blocks(driver, st.in(rk.data(), rk.size()), st.in(in.data(), in.size()), n_blocks, rounds,
                       st.out(out.data(), out.size()), nr);
        st.finish();
    }
    return wrap_bits(out, flat_noise(std::move(out_noise), n_blocks * 128), L, params().max_noise_sq);
}

// ---------------------------------------------------------------------------------------------
// AES-128-CTR with public counters (main.rs:108-128)
// ---------------------------------------------------------------------------------------------
std::vector<std::vector<NoiseLevel>> aes_ctr_noise_schedule(const std::vector<NoiseLevel> &rk, const CtrPlan &plan,
                                                            size_t n_blocks, int rounds, uint64_t max, int nr) {
    const std::vector<NoiseLevel> triv(128, NoiseLevel::trivial());
    std::vector<std::vector<NoiseLevel>> out(n_blocks);
    if (rounds != 1) {
        for (auto &o : out) o = aes_noise_schedule(rk, triv, rounds, max, nr);
        return out;
    }
    // one round: ARK(rk0) on trivial bits, SubBytes 8 -> 8 of every group (noise^2 = 8, one id per output
    // bit of a GROUP), ShiftRows, ARK(the last round key)
    std::vector<NoiseLevel> sb(plan.groups.size() * 8);
    for (auto &x : sb) x = NoiseLevel::with_noise_level(8, next_ct_id());
    for (size_t blk = 0; blk < n_blocks; blk++) {
        out[blk].resize(128);
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++)
                for (int b = 0; b < 8; b++) {
                    NoiseLevel v = sb[(size_t)plan.map[blk * 16 + 4 * ((c + r) % 4) + r] * 8 + b];
                    v.add_assign(rk[((4 * nr + c) * 4 + r) * 8 + b], max);
                    out[blk][(4 * c + r) * 8 + b] = std::move(v);
                }
    }
    return out;
}

// argument checks and the static noise validation, before any device work
int Context::check_ctr(uint64_t first_counter, size_t n_blocks, int rounds, int key_bits) const {
    if (params().model == 2)
        throw ModelError{TAE_E_PARAM, "counter mode is not available for the shortint_1bit parameter set"};
    const int nr = require_key_bits(key_bits, AesDriver::GalMul);
    require_rounds(rounds, nr);
    if (!ctr_range_ok(first_counter, n_blocks)) throw ModelError{TAE_E_ARG, "counter range wraps past 2^64 - 1"};
    std::vector<NoiseLevel> krk((size_t)aes_words(key_bits) * 32), kbl(128, NoiseLevel::trivial());
    for (auto &x : krk) x = params().model != 1 ? NoiseLevel{1, {}} : NoiseLevel::with_noise_level(1, next_ct_id());
    block_noise_schedule(AesDriver::GalMul, krk, kbl, rounds, nr);
    return nr;
}

void Context::run_aes_ctr(const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter, size_t n_blocks, int rounds,
                          const uint8_t *data, size_t out_bytes, uint64_t *out, bool device_mem, int nr) {
    const size_t S = bit_len(), kw = (size_t)4 * (nr + 1) * 32;
    Staged st(*this, device_mem);
    engine_->aes_ctr(st.in(rk, kw * S), iv, first_counter, n_blocks, rounds, st.pub(data, out_bytes), out_bytes,
                     st.out(out, out_bytes * 8 * S), nr);
    st.finish();
}

void Context::aes_ctr_keystream_raw(const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter, size_t n_blocks,
                                    int rounds, uint64_t *out, bool device_mem, int key_bits) {
    const int nr = check_ctr(first_counter, n_blocks, rounds, key_bits);
    if (!n_blocks) return;
    run_aes_ctr(rk, iv, first_counter, n_blocks, rounds, nullptr, n_blocks * 16, out, device_mem, nr);
}

void Context::aes_ctr_transcipher_raw(const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter,
                                      const uint8_t *data, size_t len, int rounds, uint64_t *out, bool device_mem,
                                      int key_bits) {
    const size_t n_blocks = len / 16 + (len % 16 != 0);
    const int nr = check_ctr(first_counter, n_blocks, rounds, key_bits);
    if (!len) return;
    run_aes_ctr(rk, iv, first_counter, n_blocks, rounds, data, len, out, device_mem, nr);
}

std::vector<BitCt> Context::aes_ctr_transcipher(const std::vector<const BitCt *> &expanded_key, const uint8_t iv[8],
                                                uint64_t first_counter, const uint8_t *data, size_t len, int rounds,
                                                int key_bits) {
    require_key_bits(key_bits, AesDriver::GalMul);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    require_key_words(expanded_key.size(), aes_nr(key_bits), "expanded key");
    const size_t L = bit_len();
    for (const BitCt *b : expanded_key)
        if (b->ct.size() != L) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
    const size_t n_blocks = len / 16 + (len % 16 != 0);
    const int nr = check_ctr(first_counter, n_blocks, rounds, key_bits);
    if (!len) return {};
    std::vector<NoiseLevel> krk(kw);
    for (size_t i = 0; i < krk.size(); i++) krk[i] = expanded_key[i]->noise;
    std::vector<std::vector<NoiseLevel>> out_noise(n_blocks);
    if (params().model == 1) {
        CtrPlan plan;
        ctr_plan(iv, first_counter, n_blocks, plan);
        out_noise = aes_ctr_noise_schedule(krk, plan, n_blocks, rounds, params().max_noise_sq, nr);
    } else {
        const std::vector<NoiseLevel> triv(128, NoiseLevel::trivial());
        for (auto &o : out_noise) o = block_noise_schedule(AesDriver::GalMul, krk, triv, rounds, nr);
    }
    std::vector<uint64_t> rk(kw * L), out(len * 8 * L);
    for (size_t i = 0; i < kw; i++) std::memcpy(&rk[i * L], expanded_key[i]->ct.data(), L * 8);
    run_aes_ctr(rk.data(), iv, first_counter, n_blocks, rounds, data, len, out.data(), false, nr);
    // xor with a public bit adds no noise
    return wrap_bits(out, flat_noise(std::move(out_noise), len * 8), L, params().max_noise_sq);
}

// ---------------------------------------------------------------------------------------------
// AES-128 inverse cipher (FIPS-197 5.3; aes_inv.hpp).  The reference has no decryption.
// ---------------------------------------------------------------------------------------------
// Metadata-only replay of decrypt_block_for_rounds for ONE block: dk [4 (nr + 1) * 32], block [128].
std::vector<NoiseLevel> aes_decrypt_noise_schedule(const std::vector<NoiseLevel> &dk, const std::vector<NoiseLevel> &block,
                                                   int rounds, uint64_t max, int nr) {
    auto key_bit = [&](int word, int byte, int bit) -> const NoiseLevel & { return dk[(word * 4 + byte) * 8 + bit]; };
    std::vector<NoiseLevel> st = block;  // index (4*col + row)*8 + bit
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++)
            for (int b = 0; b < 8; b++) st[(4 * c + r) * 8 + b].add_assign(key_bit(4 * nr + c, r, b), max);
    auto cbs_outputs = [&](int n_out) {
        std::vector<NoiseLevel> o((size_t)16 * n_out);
        for (auto &x : o) x = NoiseLevel::with_noise_level(8, next_ct_id());
        return o;
    };
    for (int round = rounds - 1; round >= 1; round--) {
        const std::vector<NoiseLevel> muls = cbs_outputs(32);  // [byte][32]
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++)
                for (int b = 0; b < 8; b++) {
                    NoiseLevel v = muls[inv_mix_src_byte(r, c, 0, true) * 32 + b];
                    for (int j = 1; j < 4; j++) v.add_assign(muls[inv_mix_src_byte(r, c, j, true) * 32 + 8 * j + b], max);
                    v.add_assign(key_bit(4 * round + c, r, b), max);
                    st[(4 * c + r) * 8 + b] = std::move(v);
                }
    }
    const std::vector<NoiseLevel> sb = cbs_outputs(8);
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++)
            for (int b = 0; b < 8; b++) {
                NoiseLevel v = sb[inv_final_src_byte(r, c) * 8 + b];
                v.add_assign(key_bit(c, r, b), max);
                st[(4 * c + r) * 8 + b] = std::move(v);
            }
    return st;
}

// The decryption-key derivation on metadata: words 0..3 and 4 nr .. 4 nr + 3 keep the expanded key's levels; every
// bit of words 4 .. 4 nr - 1 is a 4-term sum of fresh 8 -> 32 outputs (noise^2 = 32, validated), then bootstrapped.
std::vector<NoiseLevel> aes_decrypt_key_noise_schedule(const std::vector<NoiseLevel> &rk, uint64_t max, int nr) {
    std::vector<NoiseLevel> dk = rk;
    std::vector<NoiseLevel> muls((size_t)16 * (nr - 1) * 32);
    for (auto &x : muls) x = NoiseLevel::with_noise_level(8, next_ct_id());
    for (int w = 4; w < 4 * nr; w++)
        for (int r = 0; r < 4; r++)
            for (int b = 0; b < 8; b++) {
                const int blk = w / 4 - 1, c = w % 4;
                NoiseLevel v = muls[(size_t)(blk * 16 + inv_mix_src_byte(r, c, 0, false)) * 32 + b];
                for (int j = 1; j < 4; j++)
                    v.add_assign(muls[(size_t)(blk * 16 + inv_mix_src_byte(r, c, j, false)) * 32 + 8 * j + b], max);
                dk[(w * 4 + r) * 8 + b] = NoiseLevel::with_noise_level(1, next_ct_id());  // identity bootstrap
            }
    return dk;
}

// rounds < 0: the full round count of the key size.  Returns Nr.
int Context::require_inverse(int rounds, int key_bits) const {
    if (params().model != 1)
        throw ModelError{TAE_E_PARAM, "the inverse cipher runs on the 1-bit WoP-PBS parameter sets (gal-mul driver) only"};
    const int nr = require_key_bits(key_bits, AesDriver::GalMul);
    if (rounds >= 0) require_rounds(rounds, nr);
    return nr;
}

static std::vector<NoiseLevel> fresh_levels(size_t n) {
    std::vector<NoiseLevel> v(n);
    for (auto &x : v) x = NoiseLevel::with_noise_level(1, next_ct_id());
    return v;
}

static std::vector<uint64_t> gather_bits(const std::vector<const BitCt *> &bits, size_t L) {
    std::vector<uint64_t> a(bits.size() * L);
    for (size_t i = 0; i < bits.size(); i++) {
        if (bits[i]->ct.size() != L) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
        std::memcpy(&a[i * L], bits[i]->ct.data(), L * 8);
    }
    return a;
}

void Context::aes_decrypt_key_raw(const uint64_t *rk, uint64_t *dk, bool device_mem, int key_bits) {
    const int nr = require_inverse(-1, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    aes_decrypt_key_noise_schedule(fresh_levels(kw), params().max_noise_sq, nr);
    if (device_mem && rk == dk) throw ModelError{TAE_E_ARG, "the decryption key cannot be derived in place"};
    Staged st(*this, device_mem);
    engine_->aes_decrypt_key(st.in(rk, kw * bit_len()), st.out(dk, kw * bit_len()), nr);
    st.finish();
}

std::vector<BitCt> Context::aes_decrypt_key(const std::vector<const BitCt *> &expanded_key, int key_bits) {
    const int nr = require_inverse(-1, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    require_key_words(expanded_key.size(), nr, "expanded key");
    const size_t L = bit_len();
    const std::vector<uint64_t> rk = gather_bits(expanded_key, L);
    std::vector<NoiseLevel> krk(kw);
    for (size_t i = 0; i < krk.size(); i++) krk[i] = expanded_key[i]->noise;
    const std::vector<NoiseLevel> kdk = aes_decrypt_key_noise_schedule(krk, params().max_noise_sq, nr);
    std::vector<uint64_t> dk(rk.size());
    {
        Staged st(*this, false);
        engine_->aes_decrypt_key(st.in(rk.data(), rk.size()), st.out(dk.data(), dk.size()), nr);
        st.finish();
    }
    return wrap_bits(dk, kdk, L, params().max_noise_sq);
}

void Context::aes_decrypt_blocks_raw(const uint64_t *dk, const uint64_t *blocks, size_t n_blocks, int rounds,
                                     uint64_t *out, bool device_mem, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    // static validation of the fixed schedule for a derived key and fresh blocks (noise^2 = 1, own ids)
    aes_decrypt_noise_schedule(fresh_levels(kw), fresh_levels(128), rounds, params().max_noise_sq, nr);
    if (!n_blocks) return;
    const size_t len = n_blocks * 128 * bit_len();
    Staged st(*this, device_mem);
    engine_->aes_decrypt_blocks(st.in(dk, kw * bit_len()), st.in(blocks, len), n_blocks, rounds, st.out(out, len), nr);
    st.finish();
}

std::vector<BitCt> Context::aes_decrypt_blocks(const std::vector<const BitCt *> &dk,
                                               const std::vector<const BitCt *> &blocks, size_t n_blocks, int rounds,
                                               int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    require_key_words(dk.size(), nr, "decryption key");
    if (blocks.size() != n_blocks * 128) throw ModelError{TAE_E_ARG, "blocks must be 128 bits each"};
    const size_t L = bit_len();
    const std::vector<uint64_t> key = gather_bits(dk, L), in = gather_bits(blocks, L);
    std::vector<NoiseLevel> kdk(kw);
    for (size_t i = 0; i < kdk.size(); i++) kdk[i] = dk[i]->noise;
    std::vector<std::vector<NoiseLevel>> out_noise(n_blocks);
    for (size_t blk = 0; blk < n_blocks; blk++) {
        std::vector<NoiseLevel> kb(128);
        for (int i = 0; i < 128; i++) kb[i] = blocks[blk * 128 + i]->noise;
        out_noise[blk] = aes_decrypt_noise_schedule(kdk, kb, rounds, params().max_noise_sq, nr);
    }
    std::vector<uint64_t> out(in.size());
    if (n_blocks) {
        Staged st(*this, false);
        engine_->aes_decrypt_blocks(st.in(key.data(), key.size()), st.in(in.data(), in.size()), n_blocks, rounds,
                                    st.out(out.data(), out.size()), nr);
        st.finish();
    }
    return wrap_bits(out, flat_noise(std::move(out_noise), n_blocks * 128), L, params().max_noise_sq);
}

// iv || data, the public bytes both ends of the CBC pass read
static std::vector<uint8_t> cbc_public_bytes(const uint8_t iv[16], const uint8_t *data, size_t len) {
    if (len % 16 != 0) throw ModelError{TAE_E_ARG, "CBC data must be whole 16-byte blocks"};
    std::vector<uint8_t> pub(16 + len);
    std::memcpy(pub.data(), iv, 16);
    if (len) std::memcpy(pub.data() + 16, data, len);
    return pub;
}

void Context::aes_cbc_transcipher_raw(const uint64_t *dk, const uint8_t iv[16], const uint8_t *data, size_t len,
                                      int rounds, uint64_t *out, bool device_mem, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    const std::vector<uint8_t> pub = cbc_public_bytes(iv, data, len);
    aes_decrypt_noise_schedule(fresh_levels(kw), std::vector<NoiseLevel>(128, NoiseLevel::trivial()), rounds,
                               params().max_noise_sq, nr);
    if (!len) return;
    Staged st(*this, device_mem);
    engine_->aes_cbc_transcipher(st.in(dk, kw * bit_len()), st.pub(pub.data(), pub.size()), len / 16, rounds,
                                 st.out(out, len * 8 * bit_len()), nr);
    st.finish();
}

std::vector<BitCt> Context::aes_cbc_transcipher(const std::vector<const BitCt *> &dk, const uint8_t iv[16],
                                                const uint8_t *data, size_t len, int rounds, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    require_key_words(dk.size(), nr, "decryption key");
    const size_t L = bit_len();
    const std::vector<uint64_t> key = gather_bits(dk, L);
    const std::vector<uint8_t> pub = cbc_public_bytes(iv, data, len);
    std::vector<NoiseLevel> kdk(kw);
    for (size_t i = 0; i < kdk.size(); i++) kdk[i] = dk[i]->noise;
    const size_t n_blocks = len / 16;
    const std::vector<NoiseLevel> triv(128, NoiseLevel::trivial());
    std::vector<std::vector<NoiseLevel>> out_noise(n_blocks);
    for (auto &o : out_noise) o = aes_decrypt_noise_schedule(kdk, triv, rounds, params().max_noise_sq, nr);
    if (!len) return {};
    std::vector<uint64_t> out(len * 8 * L);
    {
        Staged st(*this, false);
        engine_->aes_cbc_transcipher(st.in(key.data(), key.size()), st.pub(pub.data(), pub.size()), n_blocks, rounds,
                                     st.out(out.data(), out.size()), nr);
        st.finish();
    }
    // xor with a public bit adds no noise
    return wrap_bits(out, flat_noise(std::move(out_noise), len * 8), L, params().max_noise_sq);
}

// ---------------------------------------------------------------------------------------------
// XTS-AES decryption of a public ciphertext (IEEE 1619; aes_xts.hpp).  The reference has no XTS.
// ---------------------------------------------------------------------------------------------
std::vector<NoiseLevel> aes_xts_tweak_noise_schedule(const std::vector<NoiseLevel> &rk2, int rounds, uint64_t max,
                                                     int nr) {
    // the cipher's output (8 + the last round key's bit) is validated by the schedule; the identity bootstrap
    // then gives noise^2 = 1 with fresh ids, whatever went in
    aes_noise_schedule(rk2, std::vector<NoiseLevel>(128, NoiseLevel::trivial()), rounds, max, nr);
    return fresh_levels(128);
}

std::vector<NoiseLevel> aes_xts_noise_schedule(const std::vector<NoiseLevel> &dk1, const std::vector<NoiseLevel> &tweak,
                                               uint64_t j, int rounds, uint64_t max, int nr) {
    std::vector<int16_t> rows[128];
    xts_rows_of(j, rows);
    std::vector<NoiseLevel> mask(128);
    for (int o = 0; o < 128; o++) {
        NoiseLevel v = tweak[rows[o][0]];  // x^(i + j) != 0 and A_j is invertible: no row is empty
        for (size_t q = 1; q < rows[o].size(); q++) v.add_assign(tweak[rows[o][q]], max);
        mask[o] = std::move(v);
    }
    std::vector<NoiseLevel> out = aes_decrypt_noise_schedule(dk1, mask, rounds, max, nr);
    for (int o = 0; o < 128; o++) out[o].add_assign(mask[o], max);
    return out;
}

namespace {
// the blocks of the units in order, equal tweaks merged
struct XtsFlat {
    std::vector<uint8_t> tweaks, data;  // [n_tweaks][16], [nb][16]
    std::vector<int32_t> tweak_of;      // [nb]
    std::vector<uint64_t> block_index;  // [nb]
};

int32_t xts_tweak_slot(std::vector<uint8_t> &tweaks, const uint8_t tweak[16]) {
    const size_t n = tweaks.size() / 16;
    for (size_t i = 0; i < n; i++)
        if (!std::memcmp(&tweaks[16 * i], tweak, 16)) return (int32_t)i;
    tweaks.insert(tweaks.end(), tweak, tweak + 16);
    return (int32_t)n;
}

XtsFlat xts_flatten(const std::vector<Context::XtsUnitIn> &units) {
    XtsFlat f;
    for (const Context::XtsUnitIn &u : units) {
        if (!u.len || u.len % 16)
            throw ModelError{TAE_E_PARAM, "an XTS data unit is a positive number of whole 16-byte blocks "
                                          "(ciphertext stealing is not supported)"};
        if (!u.data) throw ModelError{TAE_E_ARG, "null unit data"};
        const uint64_t blocks = u.len / 16;
        if (u.first_block + (blocks - 1) < u.first_block) throw ModelError{TAE_E_ARG, "block range wraps past 2^64 - 1"};
        const int32_t slot = xts_tweak_slot(f.tweaks, u.tweak);
        for (uint64_t b = 0; b < blocks; b++) {
            f.tweak_of.push_back(slot);
            f.block_index.push_back(u.first_block + b);
        }
        f.data.insert(f.data.end(), u.data, u.data + u.len);
    }
    return f;
}

// the block index of the call with the largest row weight (the first of them)
uint64_t xts_heaviest_block(const std::vector<uint64_t> &block_index) {
    std::vector<uint64_t> distinct = block_index;
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    uint64_t at = distinct.front();
    int w = 0;
    for (uint64_t j : distinct) {
        const int wj = xts_row_weight(j);
        if (wj > w) {
            w = wj;
            at = j;
        }
    }
    return at;
}
}  // namespace

void Context::aes_xts_tweaks_raw(const uint64_t *rk2, const uint8_t *tweaks, size_t n, int rounds, uint64_t *out,
                                 bool device_mem, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32, S = bit_len(), block_len = 128 * S;
    aes_xts_tweak_noise_schedule(fresh_levels(kw), rounds, params().max_noise_sq, nr);
    if (!n) return;
    std::vector<uint8_t> distinct;
    std::vector<int32_t> slot(n);
    for (size_t i = 0; i < n; i++) slot[i] = xts_tweak_slot(distinct, tweaks + 16 * i);
    const size_t nd = distinct.size() / 16;
    Staged st(*this, device_mem);
    DevBuf<uint64_t> d_T(nd * block_len);  // the distinct tweaks, each copied to its places in the result
    uint64_t *dst = st.out(out, n * block_len);
    engine_->aes_xts_tweaks(st.in(rk2, kw * S), st.pub(distinct.data(), distinct.size()), nd, rounds, d_T, nr);
    for (size_t i = 0; i < n; i++)
        hip_check(hipMemcpyAsync(dst + i * block_len, d_T + (size_t)slot[i] * block_len, block_len * 8,
                                 hipMemcpyDeviceToDevice, engine_->stream()),
                  "place tweak");
    st.finish();
}

void Context::xts_masks_raw(const uint64_t *tweak_cts, size_t n_units, const int32_t *unit_of_block,
                            const uint64_t *block_index, size_t nb, uint64_t *masks, bool device_mem) {
    if (params().model != 1) throw ModelError{TAE_E_PARAM, "XTS runs on the 1-bit WoP-PBS parameter sets only"};
    for (size_t b = 0; b < nb; b++)
        if (unit_of_block[b] < 0 || (size_t)unit_of_block[b] >= n_units)
            throw ModelError{TAE_E_ARG, "a block's data unit is outside 0..n_units-1"};
    if (!nb) return;
    const RowPlan plan = xts_plan(unit_of_block, block_index, nb);
    const size_t block_len = 128 * bit_len();
    Staged st(*this, device_mem);
    engine_->aes_xts_masks(st.in(tweak_cts, n_units * block_len), n_units, plan, st.out(masks, nb * block_len));
    st.finish();
}

// the flattened blocks of an XTS call through the engine, on arrays a staging scope has placed
static void xts_engine_call(Engine &e, const uint64_t *d_dk1, const uint64_t *d_rk2, const uint8_t *d_tweaks,
                            const uint8_t *d_data, const XtsFlat &f, int rounds, uint64_t *d_out, int nr) {
    e.aes_xts_transcipher(d_dk1, d_rk2, d_tweaks, f.tweaks.size() / 16, f.tweak_of.data(), f.block_index.data(), d_data,
                          f.block_index.size(), rounds, d_out, nr);
}

void Context::aes_xts_transcipher_raw(const uint64_t *dk1, const uint64_t *rk2, const std::vector<XtsUnitIn> &units,
                                      int rounds, uint64_t *out, bool device_mem, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    const XtsFlat f = xts_flatten(units);
    const uint64_t max = params().max_noise_sq;
    const std::vector<NoiseLevel> tweak = aes_xts_tweak_noise_schedule(fresh_levels(kw), rounds, max, nr);
    if (f.block_index.empty()) return;
    aes_xts_noise_schedule(fresh_levels(kw), tweak, xts_heaviest_block(f.block_index), rounds, max, nr);
    const size_t S = bit_len();
    Staged st(*this, device_mem);
    xts_engine_call(*engine_, st.in(dk1, kw * S), st.in(rk2, kw * S), st.pub(f.tweaks.data(), f.tweaks.size()),
                    st.pub(f.data.data(), f.data.size()), f, rounds, st.out(out, f.block_index.size() * 128 * S), nr);
    st.finish();
}

std::vector<BitCt> Context::aes_xts_transcipher(const std::vector<const BitCt *> &dk1,
                                                const std::vector<const BitCt *> &ek2,
                                                const std::vector<XtsUnitIn> &units, int rounds, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    require_key_words(dk1.size(), nr, "decryption key");
    require_key_words(ek2.size(), nr, "tweak key");
    const XtsFlat f = xts_flatten(units);
    const size_t L = bit_len(), nb = f.block_index.size();
    const std::vector<uint64_t> key1 = gather_bits(dk1, L), key2 = gather_bits(ek2, L);
    std::vector<NoiseLevel> kdk(kw), krk(kw);
    for (size_t i = 0; i < kw; i++) {
        kdk[i] = dk1[i]->noise;
        krk[i] = ek2[i]->noise;
    }
    const uint64_t max = params().max_noise_sq;
    std::vector<std::vector<NoiseLevel>> tweak(f.tweaks.size() / 16), out_noise(nb);
    for (auto &t : tweak) t = aes_xts_tweak_noise_schedule(krk, rounds, max, nr);
    for (size_t b = 0; b < nb; b++)
        out_noise[b] = aes_xts_noise_schedule(kdk, tweak[f.tweak_of[b]], f.block_index[b], rounds, max, nr);
    if (!nb) return {};
    std::vector<uint64_t> out(nb * 128 * L);
    {
        Staged st(*this, false);
        xts_engine_call(*engine_, st.in(key1.data(), key1.size()), st.in(key2.data(), key2.size()),
                        st.pub(f.tweaks.data(), f.tweaks.size()), st.pub(f.data.data(), f.data.size()), f, rounds,
                        st.out(out.data(), out.size()), nr);
        st.finish();
    }
    // xor with a public bit adds no noise
    return wrap_bits(out, flat_noise(std::move(out_noise), nb * 128), L, max);
}

// fhe_sbox_gal_mul_pbs::key_schedule (:134-164) with ByteT::{sbox_substitute, bootstrap_assign}
// (fhe_impls/shortint_woppbs_1bit.rs:18-45): words 0..3 = key; word i>=4 from words i-4, i-1
// (SubWord(RotWord) + Rcon when i%4 == 0), then every bit of word i is bootstrapped (identity LUT).
std::vector<BitCt> Context::aes_key_schedule(const std::vector<const BitCt *> &key, AesDriver driver) {
    if (key.size() != 128) throw ModelError{TAE_E_ARG, "key must be 16 bytes (128 bits)"};
    if (params().model != 1 || driver == AesDriver::SboxPbs) return sbox_pbs_key_schedule(key);
    const size_t L = params().big_len();
    std::vector<BitCt> ek(44 * 32);
    for (int i = 0; i < 128; i++) ek[i] = *key[i];
    uint64_t ftab_sbox[256], ftab_id[2] = {0, 1};
    for (int x = 0; x < 256; x++) ftab_sbox[x] = kSbox[x];
    const Lut sbox = generate_lookup_table(8, 8, ftab_sbox);
    const Lut ident = generate_lookup_table(1, 1, ftab_id);
    auto bit_at = [&](int word, int byte, int bit) -> BitCt & { return ek[(word * 4 + byte) * 8 + bit]; };
    std::vector<uint64_t> in, out;
    for (int i = 4; i < 44; i++) {
        std::vector<BitCt> w(32);
        if (i % 4 == 0) {
            // sub_word(rotate_left(ek[i-1], 1)): 4 SBOX circuit bootstraps (one batched call)
            in.assign(4 * 8 * L, 0);
            out.assign(4 * 8 * L, 0);
            for (int byte = 0; byte < 4; byte++)
                for (int b = 0; b < 8; b++)
                    std::memcpy(&in[(byte * 8 + b) * L], bit_at(i - 1, (byte + 1) % 4, b).ct.data(), L * 8);
            circuit_bootstrap_raw(in.data(), 4, 8, sbox, out.data(), false);
            for (int t = 0; t < 32; t++) {
                BitCt s = wrap(std::vector<uint64_t>(out.begin() + t * L, out.begin() + (t + 1) * L), 8);
                BitCt v = ek[(i - 4) * 32 + t];
                v.xor_assign(s);
                w[t] = std::move(v);
            }
            for (int b = 0; b < 8; b++) w[b].xor_assign(trivial((kRcon[i / 4] >> (7 - b)) & 1));
        } else {
            for (int t = 0; t < 32; t++) {
                BitCt v = ek[(i - 4) * 32 + t];
                v.xor_assign(ek[(i - 1) * 32 + t]);
                w[t] = std::move(v);
            }
        }
        // boot_word: identity circuit bootstrap of every bit (32 one-bit groups, one call)
        in.assign(32 * L, 0);
        out.assign(32 * L, 0);
        for (int t = 0; t < 32; t++) std::memcpy(&in[t * L], w[t].ct.data(), L * 8);
        circuit_bootstrap_raw(in.data(), 32, 1, ident, out.data(), false);
        for (int t = 0; t < 32; t++)
            ek[i * 32 + t] = wrap(std::vector<uint64_t>(out.begin() + t * L, out.begin() + (t + 1) * L), 1);
    }
    return ek;
}

// fhe_sbox_pbs::key_schedule (:123-171): sub_word = sbox_substitute of each byte of RotWord(ek[i-1]);
// after every 4th word the four words i-3..i are boot_word-ed.  ByteT per model:
//   8-bit (fhe_impls/shortint_woppbs_8bit.rs:17-42): both are Byte::bootstrap_with_lut (SBOX / identity
//     8 -> 8, outputs NOMINAL);
//   1-bit (fhe_impls/shortint_woppbs_1bit.rs:17-50): sbox_substitute is one 8 -> 8 circuit bootstrap
//     (outputs noise^2 = 8), bootstrap_assign one 1 -> 1 identity circuit bootstrap per bit (noise^2 = 1).
// Every bootstrap of a step goes to the device as one batched call.
std::vector<BitCt> Context::sbox_pbs_key_schedule(const std::vector<const BitCt *> &key) {
    const size_t L = bit_len();
    const bool m8 = params().model == 8;
    for (const BitCt *b : key)
        if (b->ct.size() != L) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
    std::vector<BitCt> ek(44 * 32);
    for (int i = 0; i < 128; i++) ek[i] = *key[i];
    uint64_t ftab_sbox[256], ftab_id[256];
    for (int x = 0; x < 256; x++) {
        ftab_sbox[x] = kSbox[x];
        ftab_id[x] = (uint64_t)x;
    }
    const Lut sbox = generate_lookup_table(8, 8, ftab_sbox);
    const Lut ident = m8 ? generate_lookup_table(8, 8, ftab_id) : generate_lookup_table(1, 1, ftab_id);
    if (params().model == 2) {
        // shortint_1bit ByteT (fhe_impls/shortint_1bit.rs:17-50): sbox_substitute = 8 multivariate functions
        // of the byte's bits, bootstrap_assign = one PBS per bit with the identity test vector; outputs
        // are fresh shortint ciphertexts (no bookkeeping: unchecked adds)
        const Engine &e = *engine_;
        auto boot = [&](std::vector<BitCt *> bits, bool sbox) {
            const size_t nbits = bits.size();
            std::vector<uint64_t> in(nbits * L), out(nbits * L);
            for (size_t t = 0; t < nbits; t++) std::memcpy(&in[t * L], bits[t]->ct.data(), L * 8);
            {
                Staged st(*this, false);
                const uint64_t *d_in = st.in(in.data(), in.size());
                uint64_t *d_out = st.out(out.data(), out.size());
                if (sbox)
                    engine_->s1_multivariate(d_in, nbits / 8, 8, e.s1_sbox_tvs(), 8, d_out);
                else
                    engine_->s1_bootstrap(d_in, e.s1_identity_tv(), 1, d_out, nbits);
                st.finish();
            }
            for (size_t t = 0; t < nbits; t++) *bits[t] = wrap(std::vector<uint64_t>(out.begin() + t * L, out.begin() + (t + 1) * L), 0);
        };
        auto bit_at = [&](int word, int byte, int bit) -> BitCt & { return ek[(word * 4 + byte) * 8 + bit]; };
        for (int i = 4; i < 44; i++) {
            if (i % 4 == 0) {
                std::vector<BitCt> rot(32);
                std::vector<BitCt *> rp(32);
                for (int byte = 0; byte < 4; byte++)
                    for (int b = 0; b < 8; b++) rot[byte * 8 + b] = bit_at(i - 1, (byte + 1) % 4, b);
                for (int t = 0; t < 32; t++) rp[t] = &rot[t];
                boot(rp, true);
                for (int t = 0; t < 32; t++) {
                    BitCt v = ek[(i - 4) * 32 + t];
                    v.xor_assign(rot[t]);
                    ek[i * 32 + t] = std::move(v);
                }
                for (int b = 0; b < 8; b++) ek[i * 32 + b].xor_assign(trivial((kRcon[i / 4] >> (7 - b)) & 1));
            } else {
                for (int t = 0; t < 32; t++) {
                    BitCt v = ek[(i - 4) * 32 + t];
                    v.xor_assign(ek[(i - 1) * 32 + t]);
                    ek[i * 32 + t] = std::move(v);
                }
            }
            if (i % 4 == 3) {
                std::vector<BitCt *> ws(128);
                for (int t = 0; t < 128; t++) ws[t] = &ek[(i - 3) * 32 + t];
                boot(ws, false);
            }
        }
        return ek;
    }
    auto boot = [&](std::vector<BitCt *> bits, const Lut &lut) {  // groups of lut.input_bits, in place
        const int n_in = lut.input_bits;
        const size_t groups = bits.size() / n_in;
        std::vector<uint64_t> in(bits.size() * L), out(bits.size() * L);
        for (size_t t = 0; t < bits.size(); t++) std::memcpy(&in[t * L], bits[t]->ct.data(), L * 8);
        circuit_bootstrap_raw(in.data(), groups, n_in, lut, out.data(), false);
        // noise: shortint NOMINAL (8-bit); NOMINAL * input_bit_count (1-bit, shortint_woppbs_1bit.rs:322-325)
        for (size_t t = 0; t < bits.size(); t++)
            *bits[t] = wrap(std::vector<uint64_t>(out.begin() + t * L, out.begin() + (t + 1) * L), m8 ? 1 : n_in);
    };
    auto bit_at = [&](int word, int byte, int bit) -> BitCt & { return ek[(word * 4 + byte) * 8 + bit]; };
    for (int i = 4; i < 44; i++) {
        if (i % 4 == 0) {
            std::vector<BitCt> rot(32);
            std::vector<BitCt *> rp(32);
            for (int byte = 0; byte < 4; byte++)
                for (int b = 0; b < 8; b++) rot[byte * 8 + b] = bit_at(i - 1, (byte + 1) % 4, b);
            for (int t = 0; t < 32; t++) rp[t] = &rot[t];
            boot(rp, sbox);
            for (int t = 0; t < 32; t++) {
                BitCt v = ek[(i - 4) * 32 + t];
                v.xor_assign(rot[t]);
                ek[i * 32 + t] = std::move(v);
            }
            for (int b = 0; b < 8; b++) ek[i * 32 + b].xor_assign(trivial((kRcon[i / 4] >> (7 - b)) & 1));
        } else {
            for (int t = 0; t < 32; t++) {
                BitCt v = ek[(i - 4) * 32 + t];
                v.xor_assign(ek[(i - 1) * 32 + t]);
                ek[i * 32 + t] = std::move(v);
            }
        }
        if (i % 4 == 3) {
            std::vector<BitCt *> ws(128);
            for (int t = 0; t < 128; t++) ws[t] = &ek[(i - 3) * 32 + t];
            boot(ws, ident);
        }
    }
    return ek;
}

void Context::aes_key_schedule_raw(const uint64_t *key, uint64_t *expanded, bool device_mem, AesDriver driver) {
    const size_t L = bit_len();
    std::vector<uint64_t> hk(128 * L);
    if (device_mem) {
        std::lock_guard<std::mutex> g(mu_);  // the engine (and its device) is shared: same lock as every entry
        engine_->order_after_caller();
        // on the engine stream, which waits for the caller's stream (a plain hipMemcpy runs on the null
        // stream, which does not wait for a non-blocking caller stream)
        hip_check(hipMemcpyAsync(hk.data(), key, hk.size() * 8, hipMemcpyDeviceToHost, engine_->stream()),
                  "download key");
        engine_->synchronize();
    } else {
        std::memcpy(hk.data(), key, hk.size() * 8);
    }
    std::vector<BitCt> kb(128);
    std::vector<const BitCt *> kp(128);
    for (int i = 0; i < 128; i++) {
        kb[i] = wrap(std::vector<uint64_t>(hk.begin() + i * L, hk.begin() + (i + 1) * L), 1);  // fresh
        kp[i] = &kb[i];
    }
    const std::vector<BitCt> ek = aes_key_schedule(kp, driver);
    std::vector<uint64_t> he(44 * 32 * L);
    for (size_t i = 0; i < ek.size(); i++) std::memcpy(&he[i * L], ek[i].ct.data(), L * 8);
    if (device_mem) {
        std::lock_guard<std::mutex> g(mu_);
        hip_check(hipMemcpyAsync(expanded, he.data(), he.size() * 8, hipMemcpyHostToDevice, engine_->stream()),
                  "upload expanded key");
        engine_->synchronize();
    } else
        std::memcpy(expanded, he.data(), he.size() * 8);
}

// ---------------------------------------------------------------------------------------------
// Key expansion on the device for 128 / 192 / 256-bit keys (FIPS-197 5.2, figure 11; Engine::aes_key_expand)
// ---------------------------------------------------------------------------------------------
// The expansion on metadata: key [nk*32] -> rk [4 (nk + 7) * 32].  Words below nk keep the key's levels and ids.
// The word before its bootstrap is rk[i-nk] + a fresh SubWord output (noise^2 = 8) on SubWord steps and
// rk[i-nk] + rk[i-1] otherwise (Rcon is trivial), validated; every word from nk on leaves the identity bootstrap
// at noise^2 = 1 with fresh ids.
std::vector<NoiseLevel> aes_key_expand_noise_schedule(const std::vector<NoiseLevel> &key, int nk, uint64_t max) {
    const int words = 4 * (nk + 7);
    std::vector<NoiseLevel> rk((size_t)words * 32);
    std::copy(key.begin(), key.end(), rk.begin());
    for (int i = nk; i < words; i++) {
        const bool sub = i % nk == 0 || (nk == 8 && i % 8 == 4);
        for (int t = 0; t < 32; t++) {
            NoiseLevel v = rk[(size_t)(i - nk) * 32 + t];
            v.add_assign(sub ? NoiseLevel::with_noise_level(8, next_ct_id()) : rk[(size_t)(i - 1) * 32 + t], max);
        }
        for (int t = 0; t < 32; t++) rk[(size_t)i * 32 + t] = NoiseLevel::with_noise_level(1, next_ct_id());
    }
    return rk;
}

// the scope of the device key expansion; returns Nk
int Context::require_key_expand(int key_bits) const {
    if (!aes_key_bits_ok(key_bits)) throw ModelError{TAE_E_PARAM, "key_bits must be 128, 192 or 256"};
    if (params().model != 1)
        throw ModelError{TAE_E_PARAM,
                         "the device key expansion runs on the 1-bit WoP-PBS parameter sets (gal-mul driver) only"};
    return aes_nk(key_bits);
}

void Context::aes_key_expand_raw(const uint64_t *key, uint64_t *expanded, bool device_mem, int key_bits) {
    const int nk = require_key_expand(key_bits);
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    aes_key_expand_noise_schedule(fresh_levels((size_t)nk * 32), nk, params().max_noise_sq);
    Staged st(*this, device_mem);
    uint64_t *d_rk = st.out(expanded, kw * L);
    if (!device_mem) {  // the key is uploaded into its place, words 0 .. nk - 1, and expanded there
        hip_check(hipMemcpyAsync(d_rk, key, (size_t)nk * 32 * L * 8, hipMemcpyHostToDevice, engine_->stream()), "upload key");
        key = d_rk;
    }
    engine_->aes_key_expand(key, nk, d_rk);
    st.finish();
}

std::vector<BitCt> Context::aes_key_expand(const std::vector<const BitCt *> &key, int key_bits) {
    const int nk = require_key_expand(key_bits);
    if (key.size() != (size_t)nk * 32)
        throw ModelError{TAE_E_ARG, "key must be " + std::to_string(4 * nk) + " bytes (" + std::to_string(32 * nk) + " bits)"};
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    const std::vector<uint64_t> hk = gather_bits(key, L);
    std::vector<NoiseLevel> kn(key.size());
    for (size_t i = 0; i < kn.size(); i++) kn[i] = key[i]->noise;
    const std::vector<NoiseLevel> krk = aes_key_expand_noise_schedule(kn, nk, params().max_noise_sq);
    std::vector<uint64_t> rk(kw * L);
    {
        Staged st(*this, false);
        uint64_t *d_rk = st.out(rk.data(), rk.size());  // the key in its place, as in aes_key_expand_raw
        hip_check(hipMemcpyAsync(d_rk, hk.data(), hk.size() * 8, hipMemcpyHostToDevice, engine_->stream()), "upload key");
        engine_->aes_key_expand(d_rk, nk, d_rk);
        st.finish();
    }
    return wrap_bits(rk, krk, L, params().max_noise_sq);
}

// ---------------------------------------------------------------------------------------------
// Multi-key batches: key tables [n_keys][W*32][L].  The reference has one key.
// ---------------------------------------------------------------------------------------------
// the scope of the multi-key entry points; rounds < 0: no round count to check.  Returns Nr.
int Context::require_multi(int key_bits, int rounds) const {
    if (!aes_key_bits_ok(key_bits)) throw ModelError{TAE_E_PARAM, "key_bits must be 128, 192 or 256"};
    if (params().model != 1)
        throw ModelError{TAE_E_PARAM, "multi-key batches run on the 1-bit WoP-PBS parameter sets (gal-mul driver) only"};
    const int nr = aes_nr(key_bits);
    if (rounds >= 0) require_rounds(rounds, nr);
    return nr;
}

static void require_slots(const int32_t *slots, size_t n, size_t n_keys) {
    for (size_t i = 0; i < n; i++)
        if (slots[i] < 0 || (uint64_t)slots[i] >= n_keys)
            throw ModelError{TAE_E_ARG, "key slot " + std::to_string(slots[i]) + " outside 0.." + std::to_string(n_keys) + "-1"};
}

// the slots a call refers to, ascending; `slots` is rewritten to indices into that list
static std::vector<int32_t> compact_slots(std::vector<int32_t> &slots) {
    std::vector<int32_t> used(slots);
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    for (int32_t &s : slots) s = (int32_t)(std::lower_bound(used.begin(), used.end(), s) - used.begin());
    return used;
}

const uint64_t *Context::Staged::table(const uint64_t *table, std::vector<int32_t> &slots, size_t stride) {
    if (dev_) return table;
    const std::vector<int32_t> used = compact_slots(slots);
    uint64_t *d_tab = alloc<uint64_t>(used.size() * stride);
    for (size_t j = 0; j < used.size(); j++)
        hip_check(hipMemcpyAsync(d_tab + j * stride, table + (size_t)used[j] * stride, stride * 8, hipMemcpyHostToDevice,
                                 e_.stream()),
                  "upload key slot");
    return d_tab;
}

void Context::aes_key_expand_multi_raw(const uint64_t *keys, size_t n_keys, uint64_t *table, bool device_mem,
                                       int key_bits) {
    require_multi(key_bits, -1);
    const int nk = aes_nk(key_bits);
    if (!n_keys) return;
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    aes_key_expand_noise_schedule(fresh_levels((size_t)nk * 32), nk, params().max_noise_sq);
    Staged st(*this, device_mem);
    engine_->aes_key_expand_multi(st.in(keys, n_keys * (size_t)nk * 32 * L), nk, n_keys, st.out(table, n_keys * kw * L));
    st.finish();
}

std::vector<BitCt> Context::aes_key_expand_multi(const std::vector<const BitCt *> &keys, size_t n_keys, int key_bits) {
    require_multi(key_bits, -1);
    const int nk = aes_nk(key_bits);
    if (keys.size() != n_keys * (size_t)nk * 32) throw ModelError{TAE_E_ARG, "keys must be n_keys * key_bits bits"};
    if (!n_keys) return {};
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    const std::vector<uint64_t> hk = gather_bits(keys, L);
    std::vector<NoiseLevel> noise;  // the single-key bookkeeping, key by key
    noise.reserve(n_keys * kw);
    for (size_t k = 0; k < n_keys; k++) {
        std::vector<NoiseLevel> kn((size_t)nk * 32);
        for (size_t i = 0; i < kn.size(); i++) kn[i] = keys[k * kn.size() + i]->noise;
        for (NoiseLevel &x : aes_key_expand_noise_schedule(kn, nk, params().max_noise_sq)) noise.push_back(std::move(x));
    }
    std::vector<uint64_t> tab(n_keys * kw * L);
    {
        Staged st(*this, false);
        engine_->aes_key_expand_multi(st.in(hk.data(), hk.size()), nk, n_keys, st.out(tab.data(), tab.size()));
        st.finish();
    }
    return wrap_bits(tab, std::move(noise), L, params().max_noise_sq);
}

void Context::aes_decrypt_key_multi_raw(const uint64_t *table, size_t n_keys, uint64_t *dtable, bool device_mem,
                                        int key_bits) {
    const int nr = require_multi(key_bits, -1);
    if (!n_keys) return;
    const size_t kw = (size_t)aes_words(key_bits) * 32, len = n_keys * kw * bit_len();
    aes_decrypt_key_noise_schedule(fresh_levels(kw), params().max_noise_sq, nr);
    if (table == dtable) throw ModelError{TAE_E_ARG, "the decryption keys cannot be derived in place"};
    Staged st(*this, device_mem);
    engine_->aes_decrypt_key_multi(st.in(table, len), n_keys, st.out(dtable, len), nr);
    st.finish();
}

void Context::aes_blocks_multi_raw(bool inverse, const uint64_t *table, size_t n_keys, const int32_t *key_of,
                                   const uint64_t *blocks, size_t n_blocks, int rounds, uint64_t *out, bool device_mem,
                                   int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    if (!n_blocks) return;
    if (!n_keys) throw ModelError{TAE_E_ARG, "blocks but no keys"};
    require_slots(key_of, n_blocks, n_keys);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    // the single-key schedule: batching keys mixes no ciphertexts of different keys
    if (inverse)
        aes_decrypt_noise_schedule(fresh_levels(kw), fresh_levels(128), rounds, params().max_noise_sq, nr);
    else
        aes_noise_schedule(fresh_levels(kw), fresh_levels(128), rounds, params().max_noise_sq, nr);
    const size_t len = n_blocks * 128 * bit_len();
    std::vector<int32_t> slots(key_of, key_of + n_blocks);
    Staged st(*this, device_mem);
    const uint64_t *d_tab = st.table(table, slots, kw * bit_len()), *d_in = st.in(blocks, len);
    uint64_t *d_out = st.out(out, len);
    if (inverse)
        engine_->aes_decrypt_blocks_multi(d_tab, slots.data(), d_in, n_blocks, rounds, d_out, nr);
    else
        engine_->aes_encrypt_blocks_multi(d_tab, slots.data(), d_in, n_blocks, rounds, d_out, nr);
    st.finish();
}

// the flattened blocks of the streams and their public bytes in output order (empty: every stream asks for the
// keystream); slot and range errors are TAE_E_ARG
static void ctr_streams(const std::vector<Context::CtrStreamIn> &streams, size_t n_keys, std::vector<CtrBlock> &blocks,
                        std::vector<uint8_t> &pub, size_t &total) {
    std::vector<CtrStream> ss(streams.size());
    total = 0;
    bool any = false;
    for (size_t i = 0; i < streams.size(); i++) {
        ss[i] = streams[i].s;
        total += ss[i].len;
        any = any || (ss[i].len && streams[i].data);
    }
    switch (ctr_flatten(ss.data(), ss.size(), (int64_t)n_keys, blocks)) {
        case CTR_FLAT_SLOT: throw ModelError{TAE_E_ARG, "a stream's key slot is outside 0..n_keys-1"};
        case CTR_FLAT_WRAP: throw ModelError{TAE_E_ARG, "counter range wraps past 2^64 - 1"};
        default: break;
    }
    pub.clear();
    if (!any) return;
    pub.assign(total, 0);  // a stream without data adds zeros: its keystream
    size_t at = 0;
    for (const Context::CtrStreamIn &st : streams) {
        if (st.s.len && st.data) std::memcpy(pub.data() + at, st.data, st.s.len);
        at += st.s.len;
    }
}

void Context::aes_ctr_multi_raw(const uint64_t *table, size_t n_keys, const std::vector<CtrStreamIn> &streams,
                                int rounds, uint64_t *out, bool device_mem, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    std::vector<CtrBlock> blocks;
    std::vector<uint8_t> pub;
    size_t total = 0;
    ctr_streams(streams, n_keys, blocks, pub, total);
    if (blocks.empty()) return;
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    aes_noise_schedule(fresh_levels(kw), std::vector<NoiseLevel>(128, NoiseLevel::trivial()), rounds,
                       params().max_noise_sq, nr);
    std::vector<int32_t> slots(blocks.size());
    for (size_t i = 0; i < blocks.size(); i++) slots[i] = blocks[i].slot;
    Staged st(*this, device_mem);
    const uint64_t *d_tab = st.table(table, slots, kw * bit_len());
    for (size_t i = 0; i < blocks.size(); i++) blocks[i].slot = slots[i];
    engine_->aes_ctr_multi(d_tab, blocks, rounds, st.pub(pub.data(), pub.size()), st.out(out, total * 8 * bit_len()), nr);
    st.finish();
}

// the referenced slots of a handle table as a compact host table, with the noise of every bit; `slots` is renumbered
static std::vector<uint64_t> gather_slots(const Context::BitAt &table, std::vector<int32_t> &slots, size_t kw, size_t L,
                                          std::vector<std::vector<NoiseLevel>> &noise) {
    const std::vector<int32_t> used = compact_slots(slots);
    std::vector<uint64_t> tab(used.size() * kw * L);
    noise.assign(used.size(), std::vector<NoiseLevel>(kw));
    for (size_t j = 0; j < used.size(); j++)
        for (size_t i = 0; i < kw; i++) {
            const BitCt *b = table((size_t)used[j] * kw + i);
            if (b->ct.size() != L) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
            std::memcpy(&tab[(j * kw + i) * L], b->ct.data(), L * 8);
            noise[j][i] = b->noise;
        }
    return tab;
}

std::vector<BitCt> Context::aes_ctr_multi(const BitAt &table, size_t n_keys, const std::vector<CtrStreamIn> &streams,
                                          int rounds, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    std::vector<CtrBlock> blocks;
    std::vector<uint8_t> pub;
    size_t total = 0;
    ctr_streams(streams, n_keys, blocks, pub, total);
    if (blocks.empty()) return {};
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    std::vector<int32_t> slots(blocks.size());
    for (size_t i = 0; i < blocks.size(); i++) slots[i] = blocks[i].slot;
    std::vector<std::vector<NoiseLevel>> knoise;
    const std::vector<uint64_t> tab = gather_slots(table, slots, kw, L, knoise);
    // the bookkeeping of aes_ctr_transcipher, stream by stream
    std::vector<NoiseLevel> noise;
    noise.reserve(total * 8);
    size_t b0 = 0;
    for (const CtrStreamIn &st : streams) {
        if (!st.s.len) continue;
        const size_t nb = st.s.len / 16 + (st.s.len % 16 != 0);
        CtrPlan plan;
        ctr_plan(st.s.iv, st.s.first_counter, nb, plan);
        const std::vector<std::vector<NoiseLevel>> on =
            aes_ctr_noise_schedule(knoise[(size_t)slots[b0]], plan, nb, rounds, params().max_noise_sq, nr);
        for (size_t i = 0; i < st.s.len * 8; i++) noise.push_back(on[i / 128][i % 128]);
        b0 += nb;
    }
    for (size_t i = 0; i < blocks.size(); i++) blocks[i].slot = slots[i];
    std::vector<uint64_t> out(total * 8 * L);
    {
        Staged st(*this, false);
        engine_->aes_ctr_multi(st.in(tab.data(), tab.size()), blocks, rounds, st.pub(pub.data(), pub.size()),
                               st.out(out.data(), out.size()), nr);
        st.finish();
    }
    // xor with a public bit adds no noise
    return wrap_bits(out, std::move(noise), L, params().max_noise_sq);
}

// per block of the flattened streams: slot, the ciphertext block and the block before it (the iv first)
static void cbc_streams(const std::vector<Context::CbcStreamIn> &streams, size_t n_keys, std::vector<int32_t> &slots,
                        std::vector<uint8_t> &cur_prev) {
    size_t nb = 0;
    for (const Context::CbcStreamIn &st : streams) {
        if (st.len % 16 != 0) throw ModelError{TAE_E_ARG, "CBC data must be whole 16-byte blocks"};
        if (st.len && (st.slot < 0 || (uint64_t)st.slot >= n_keys))
            throw ModelError{TAE_E_ARG, "a stream's key slot is outside 0..n_keys-1"};
        nb += st.len / 16;
    }
    slots.clear();
    cur_prev.assign(nb * 32, 0);  // [nb][16] ciphertext blocks, then [nb][16] previous blocks
    size_t b = 0;
    for (const Context::CbcStreamIn &st : streams)
        for (size_t i = 0; i < st.len / 16; i++, b++) {
            slots.push_back(st.slot);
            std::memcpy(&cur_prev[b * 16], st.data + 16 * i, 16);
            std::memcpy(&cur_prev[(nb + b) * 16], i ? st.data + 16 * (i - 1) : st.iv, 16);
        }
}

void Context::aes_cbc_multi_raw(const uint64_t *dtable, size_t n_keys, const std::vector<CbcStreamIn> &streams,
                                int rounds, uint64_t *out, bool device_mem, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    std::vector<int32_t> slots;
    std::vector<uint8_t> pub;
    cbc_streams(streams, n_keys, slots, pub);
    const size_t nb = slots.size(), kw = (size_t)aes_words(key_bits) * 32;
    if (!nb) return;
    aes_decrypt_noise_schedule(fresh_levels(kw), std::vector<NoiseLevel>(128, NoiseLevel::trivial()), rounds,
                               params().max_noise_sq, nr);
    Staged st(*this, device_mem);
    const uint64_t *d_tab = st.table(dtable, slots, kw * bit_len());
    const uint8_t *d_pub = st.pub(pub.data(), pub.size());
    engine_->aes_cbc_transcipher_multi(d_tab, slots.data(), d_pub, d_pub + nb * 16, nb, rounds,
                                       st.out(out, nb * 128 * bit_len()), nr);
    st.finish();
}

std::vector<BitCt> Context::aes_cbc_multi(const BitAt &dtable, size_t n_keys, const std::vector<CbcStreamIn> &streams,
                                          int rounds, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    std::vector<int32_t> slots;
    std::vector<uint8_t> pub;
    cbc_streams(streams, n_keys, slots, pub);
    const size_t nb = slots.size(), kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    if (!nb) return {};
    std::vector<std::vector<NoiseLevel>> knoise;
    const std::vector<uint64_t> tab = gather_slots(dtable, slots, kw, L, knoise);
    const std::vector<NoiseLevel> triv(128, NoiseLevel::trivial());
    std::vector<NoiseLevel> noise;
    noise.reserve(nb * 128);
    for (size_t b = 0; b < nb; b++)
        for (NoiseLevel &x : aes_decrypt_noise_schedule(knoise[(size_t)slots[b]], triv, rounds, params().max_noise_sq, nr))
            noise.push_back(std::move(x));
    std::vector<uint64_t> out(nb * 128 * L);
    {
        Staged st(*this, false);
        const uint8_t *d_pub = st.pub(pub.data(), pub.size());
        engine_->aes_cbc_transcipher_multi(st.in(tab.data(), tab.size()), slots.data(), d_pub, d_pub + nb * 16, nb, rounds,
                                           st.out(out.data(), out.size()), nr);
        st.finish();
    }
    // xor with a public bit adds no noise
    return wrap_bits(out, std::move(noise), L, params().max_noise_sq);
}

// ---------------------------------------------------------------------------------------------
// AES-CCM decryption of public frames (RFC 3610; aes_ccm.hpp).  The reference has no CCM.
// ---------------------------------------------------------------------------------------------
CcmNoise aes_ccm_noise_schedule(const std::vector<NoiseLevel> &rk, const CcmFrame &f, int rounds, uint64_t max, int nr) {
    require_rounds(rounds, nr);
    // at one round B_0 and A_0 share their de-duplicated SubBytes outputs at the nonce positions
    if (rounds < 2) throw ModelError{TAE_E_PARAM, "CCM needs rounds >= 2"};
    require_key_words(rk.size(), nr, "expanded key");
    if (!f.n_mac() || !f.n_ctr()) throw ModelError{TAE_E_ARG, "empty CCM frame"};
    auto last_key = [&](int i) -> const NoiseLevel & { return rk[(size_t)128 * nr + i]; };
    // X' of a block: `in` is the round-0 state before round key 0
    auto x_prime = [&](std::vector<NoiseLevel> in) {
        for (int i = 0; i < 128; i++) in[i].add_assign(rk[i], max);
        return aes_noise_rounds(rk, std::move(in), rounds, max, nr, false);
    };
    const std::vector<NoiseLevel> triv(128, NoiseLevel::trivial());
    CcmNoise out;
    std::vector<std::vector<NoiseLevel>> sp(f.n_ctr());  // S'_i
    for (auto &s : sp) s = x_prime(triv);
    out.plain.resize(f.payload_len * 8);
    for (size_t q = 0; q < f.payload_len; q++)
        for (int b = 0; b < 8; b++) {
            const int i = (int)(q % 16) * 8 + b;
            NoiseLevel v = sp[1 + q / 16][i];
            v.add_assign(last_key(i), max);
            out.plain[q * 8 + b] = std::move(v);
        }
    std::vector<NoiseLevel> x = x_prime(triv);  // B_0
    for (size_t t = 1; t < f.n_mac(); t++) {
        std::vector<NoiseLevel> in(128);
        std::vector<uint64_t> levels(128);
        for (int i = 0; i < 128; i++) {
            const int64_t q = f.src[t * 16 + (size_t)(i >> 3)];
            NoiseLevel v = x[i];
            if (q >= 0)
                v.add_assign(sp[1 + (size_t)q / 16][((size_t)q % 16) * 8 + (i & 7)], max);  // Xk + P - 2 rk_nr = X' + S'
            else
                v.add_assign(last_key(i), max);  // Xk = X' + rk_nr
            levels[i] = v.noise_level_squared + rk[i].noise_level_squared;
            in[i] = std::move(v);
        }
        out.step_round0.push_back(std::move(levels));
        x = x_prime(std::move(in));
    }
    out.tag_diff.resize((size_t)8 * f.M);
    for (int i = 0; i < 8 * f.M; i++) {
        NoiseLevel v = x[i];
        v.add_assign(sp[0][i], max);  // Xk_last + S_0 - 2 rk_nr = X'_last + S'_0
        out.tag_diff[i] = std::move(v);
    }
    return out;
}

namespace {
// the frames of the streams; every refusal of the format is TAE_E_PARAM, a bad slot or a null array TAE_E_ARG
std::vector<CcmFrame> ccm_frames(const std::vector<Context::CcmStreamIn> &streams, int tag_len, size_t n_keys,
                                 std::vector<int32_t> &slots) {
    std::vector<CcmFrame> frames(streams.size());
    slots.resize(streams.size());
    for (size_t s = 0; s < streams.size(); s++) {
        const Context::CcmStreamIn &st = streams[s];
        if (!st.nonce || (!st.aad && st.aad_len) || (!st.data && st.len)) throw ModelError{TAE_E_ARG, "null frame array"};
        const size_t M = tag_len > 0 ? (size_t)tag_len : 0;
        switch (ccm_format(st.nonce, st.nonce_len, tag_len, st.aad, st.aad_len, st.len >= M ? st.len - M : 0, frames[s])) {
            case CCM_FMT_NONCE: throw ModelError{TAE_E_PARAM, "a CCM nonce is 7..13 bytes"};
            case CCM_FMT_TAG: throw ModelError{TAE_E_PARAM, "a CCM tag is 4, 6 .. 16 bytes"};
            case CCM_FMT_AAD: throw ModelError{TAE_E_PARAM, "CCM associated data of 0xFF00 bytes or more is not supported"};
            case CCM_FMT_LEN: throw ModelError{TAE_E_PARAM, "the payload length does not fit the nonce's length field"};
            default: break;
        }
        if (st.len < M) throw ModelError{TAE_E_PARAM, "CCM data is shorter than the tag"};
        if (st.slot < 0 || (uint64_t)st.slot >= n_keys)
            throw ModelError{TAE_E_ARG, "a stream's key slot is outside 0..n_keys-1"};
        slots[s] = st.slot;
    }
    return frames;
}
}  // namespace

void Context::aes_pub_keystream_multi_raw(const uint64_t *table, size_t n_keys, const int32_t *slots,
                                          const uint8_t *blocks, size_t n_blocks, int rounds, uint64_t *out,
                                          bool device_mem, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    if (!n_blocks) return;
    if (!n_keys) throw ModelError{TAE_E_ARG, "blocks but no keys"};
    require_slots(slots, n_blocks, n_keys);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    aes_noise_schedule(fresh_levels(kw), std::vector<NoiseLevel>(128, NoiseLevel::trivial()), rounds,
                       params().max_noise_sq, nr);
    std::vector<PubBlock> pb(n_blocks);
    for (size_t i = 0; i < n_blocks; i++) {
        std::memcpy(pb[i].bytes, blocks + 16 * i, 16);
        pb[i].out_byte = (int64_t)(16 * i);
        pb[i].len = 16;
    }
    std::vector<int32_t> ko(slots, slots + n_blocks);
    Staged st(*this, device_mem);
    const uint64_t *d_tab = st.table(table, ko, kw * bit_len());
    for (size_t i = 0; i < n_blocks; i++) pb[i].slot = ko[i];
    engine_->aes_pub_blocks_multi(d_tab, pb, rounds, st.out(out, n_blocks * 128 * bit_len()), nr);
    st.finish();
}

// the frames of a CCM call through the engine; host memory uploads the referenced slots alone
void Context::ccm_call(const uint64_t *table, std::vector<int32_t> slots, const std::vector<CcmFrame> &frames,
                       const std::vector<CcmStreamIn> &streams, int tag_len, int rounds, int nr, size_t key_cts,
                       uint64_t *out_plain, uint64_t *out_tag_diff, bool device_mem) {
    const size_t n = frames.size(), S = bit_len();
    size_t total = 0;
    for (const CcmFrame &f : frames) total += f.payload_len;
    Staged st(*this, device_mem);
    const uint64_t *d_tab = st.table(table, slots, key_cts * S);
    std::vector<Engine::CcmStreamIn> in(n);
    for (size_t s = 0; s < n; s++)
        in[s] = {slots[s], &frames[s], streams[s].data, streams[s].data + frames[s].payload_len};
    uint64_t *d_plain = st.out(out_plain, total * 8 * S), *d_tag = st.out(out_tag_diff, n * 8 * (size_t)tag_len * S);
    engine_->aes_ccm_transcipher(d_tab, in, rounds, nr, d_plain, d_tag);
    st.finish();
}

void Context::aes_ccm_multi_raw(const uint64_t *table, size_t n_keys, const std::vector<CcmStreamIn> &streams,
                                int tag_len, int rounds, uint64_t *out_plain, uint64_t *out_tag_diff, bool device_mem,
                                int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    if (rounds < 2) throw ModelError{TAE_E_PARAM, "CCM needs rounds >= 2"};
    std::vector<int32_t> slots;
    const std::vector<CcmFrame> frames = ccm_frames(streams, tag_len, n_keys, slots);
    if (frames.empty()) return;
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    // the levels depend on the layout alone: frames of one layout are replayed once
    std::vector<const CcmFrame *> seen;
    for (const CcmFrame &f : frames) {
        bool dup = false;
        for (const CcmFrame *o : seen) dup = dup || (o->M == f.M && o->src == f.src);
        if (dup) continue;
        seen.push_back(&f);
        aes_ccm_noise_schedule(fresh_levels(kw), f, rounds, params().max_noise_sq, nr);
    }
    ccm_call(table, slots, frames, streams, tag_len, rounds, nr, kw, out_plain, out_tag_diff, device_mem);
}

Context::CcmBits Context::aes_ccm_multi(const BitAt &table, size_t n_keys, const std::vector<CcmStreamIn> &streams,
                                        int tag_len, int rounds, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    if (rounds < 2) throw ModelError{TAE_E_PARAM, "CCM needs rounds >= 2"};
    std::vector<int32_t> slots;
    const std::vector<CcmFrame> frames = ccm_frames(streams, tag_len, n_keys, slots);
    if (frames.empty()) return {};
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len(), n = frames.size();
    std::vector<std::vector<NoiseLevel>> knoise;
    const std::vector<uint64_t> tab = gather_slots(table, slots, kw, L, knoise);
    std::vector<NoiseLevel> pn, tn;
    for (size_t s = 0; s < n; s++) {
        CcmNoise cn = aes_ccm_noise_schedule(knoise[(size_t)slots[s]], frames[s], rounds, params().max_noise_sq, nr);
        for (NoiseLevel &x : cn.plain) pn.push_back(std::move(x));
        for (NoiseLevel &x : cn.tag_diff) tn.push_back(std::move(x));
    }
    std::vector<uint64_t> plain(pn.size() * L), tag(tn.size() * L);
    ccm_call(tab.data(), slots, frames, streams, tag_len, rounds, nr, kw, plain.data(), tag.data(), false);
    // xor with a public bit adds no noise
    return {wrap_bits(plain, std::move(pn), L, params().max_noise_sq), wrap_bits(tag, std::move(tn), L, params().max_noise_sq)};
}

// ---------------------------------------------------------------------------------------------
// AES-GCM decryption of public frames (SP 800-38D; aes_gcm.hpp).  The reference has no GCM.
// ---------------------------------------------------------------------------------------------
namespace {
// the sums of a row-sum plan on metadata, every one validated; the largest level met goes to *top
std::vector<NoiseLevel> rowsum_noise(const std::vector<NoiseLevel> &src, const RowPlan &p, uint64_t max, uint64_t *top) {
    std::vector<NoiseLevel> out(p.n_rows());
    for (size_t r = 0; r < p.n_rows(); r++) {
        const size_t l = p.list_of.empty() ? r : (size_t)p.list_of[r], base = p.base_of.empty() ? 0 : (size_t)p.base_of[r];
        for (int32_t q = p.row_start[l]; q < p.row_start[l + 1]; q++) out[r].add_assign(src[base + (size_t)p.src[q]], max);
        if (top && out[r].noise_level_squared > *top) *top = out[r].noise_level_squared;
    }
    return out;
}

void require_gcm_rounds(int rounds) {
    // at one round J0 and the counter blocks share their de-duplicated SubBytes outputs at the IV positions
    if (rounds < 2) throw ModelError{TAE_E_PARAM, "GCM needs rounds >= 2"};
}

void require_powers(int n_powers) {
    if (n_powers < 1 || n_powers > kGcmMaxPowers) throw ModelError{TAE_E_PARAM, "n_powers must be in 1..=64"};
}

// one product on metadata: 7168 partial bits at 8 with fresh ids, chunk sums, a refresh, the reduction, a refresh
std::vector<NoiseLevel> product_noise(const GcmProductPlan &pp, uint64_t max, uint64_t *top_chunk, uint64_t *top_reduced) {
    std::vector<NoiseLevel> parts(kGcmParts);
    for (auto &x : parts) x = NoiseLevel::with_noise_level(8, next_ct_id());
    rowsum_noise(parts, pp.chunks, max, top_chunk);
    rowsum_noise(fresh_levels(pp.chunks.n_rows()), pp.reduce, max, top_reduced);
    return fresh_levels(128);
}

// the generations of gcm_power_schedule(n) on out.table [n * 128], whose entry 0 is the base
void power_generations_noise(GhashKeyNoise &out, int n, uint64_t max) {
    auto put = [&](int k, std::vector<NoiseLevel> v) {
        for (int i = 0; i < 128; i++) out.table[(size_t)(k - 1) * 128 + i] = std::move(v[i]);
    };
    const GcmProductPlan pp = gcm_product_plan();
    RowPlan sq = gcm_square_plan();
    for (const GcmGeneration &gen : gcm_power_schedule(n)) {
        for (int k : gen.squares) {
            sq.base_of.assign(128, (k / 2 - 1) * 128);  // the operand: power k / 2
            rowsum_noise(out.table, sq, max, &out.max_square);
            put(k, fresh_levels(128));  // refreshed even at 5: table entries must not share ids with each other
        }
        for (int k : gen.products) put(k, product_noise(pp, max, &out.max_chunk, &out.max_reduced));
    }
}

void throw_gcm_long(GcmLongStatus st) {
    switch (st) {
        case GCM_LONG_SEG: throw ModelError{TAE_E_PARAM, "seg must be in 1..=min(n_powers, 64)"};
        case GCM_LONG_STRIDES:
            throw ModelError{TAE_E_PARAM, "n_strides must be in 1..=64 and at least the frame's segments less one"};
        case GCM_LONG_NOISE: throw ModelError{TAE_E_NOISE, "a row needs more than 64 refreshed chunks"};
        default: break;
    }
}
}  // namespace

GhashKeyNoise aes_ghash_key_noise_schedule(const std::vector<NoiseLevel> &rk, int n_powers, int rounds, uint64_t max,
                                           int nr) {
    require_rounds(rounds, nr);
    require_powers(n_powers);
    require_key_words(rk.size(), nr, "expanded key");
    GhashKeyNoise out;
    out.table.resize((size_t)n_powers * 128);
    // E_K(0) is validated by the cipher's schedule; the identity bootstrap gives noise^2 = 1 with fresh ids
    aes_noise_schedule(rk, std::vector<NoiseLevel>(128, NoiseLevel::trivial()), rounds, max, nr);
    const std::vector<NoiseLevel> h1 = fresh_levels(128);
    std::copy(h1.begin(), h1.end(), out.table.begin());
    power_generations_noise(out, n_powers, max);
    return out;
}

GhashKeyNoise aes_ghash_stride_key_noise_schedule(const std::vector<NoiseLevel> &hk, size_t seg, int n_strides,
                                                  uint64_t max) {
    if (hk.empty() || hk.size() % 128) throw ModelError{TAE_E_ARG, "the power table is n_powers * 128 bits"};
    if (seg < 1 || seg > hk.size() / 128 || seg > (size_t)kGcmMaxPowers)
        throw ModelError{TAE_E_PARAM, "seg must be in 1..=min(n_powers, 64)"};
    if (n_strides < 1 || n_strides > kGcmMaxStrides) throw ModelError{TAE_E_PARAM, "n_strides must be in 1..=64"};
    GhashKeyNoise out;
    out.table.resize((size_t)n_strides * 128);
    std::copy(hk.begin() + (std::ptrdiff_t)((seg - 1) * 128), hk.begin() + (std::ptrdiff_t)(seg * 128), out.table.begin());
    power_generations_noise(out, n_strides, max);
    return out;
}

GcmNoise aes_gcm_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &hk, const GcmFrame &f,
                                int rounds, uint64_t max, int nr) {
    require_rounds(rounds, nr);
    require_gcm_rounds(rounds);
    require_key_words(rk.size(), nr, "expanded key");
    if (!f.m() || f.n_pub() < 2 || hk.size() % 128) throw ModelError{TAE_E_ARG, "empty GCM frame or a broken power table"};
    std::vector<std::vector<int32_t>> rows;
    gcm_frame_rows(f, rows);
    switch (gcm_frame_check(f, hk.size() / 128, rows)) {
        case GCM_PLAN_POWERS: throw ModelError{TAE_E_PARAM, "the frame has more hashed blocks than the power table has powers"};
        case GCM_PLAN_NOISE: throw ModelError{TAE_E_NOISE, "a tag row needs more than 64 refreshed chunks"};
        default: break;
    }
    const std::vector<NoiseLevel> triv(128, NoiseLevel::trivial());
    GcmNoise out;
    out.plain.resize(f.data_len * 8);
    for (size_t b = 0; b * 16 < f.data_len; b++) {
        const std::vector<NoiseLevel> ks = aes_noise_schedule(rk, triv, rounds, max, nr);
        for (size_t i = 0; i < 128 && (b * 16 + i / 8) < f.data_len; i++) out.plain[b * 128 + i] = ks[i];
    }
    // the chunk source array of a one-frame call: the table's first m blocks, then E(J0)
    std::vector<NoiseLevel> src(hk.begin(), hk.begin() + (std::ptrdiff_t)(f.m() * 128));
    const std::vector<NoiseLevel> j0 = aes_noise_schedule(rk, triv, rounds, max, nr);
    src.insert(src.end(), j0.begin(), j0.end());
    GcmCallPlan plan;
    const std::vector<uint8_t> no_tag((size_t)f.tag_len, 0);
    gcm_call_plan_add(plan, rows, f.m(), 0, no_tag.data());
    rowsum_noise(src, plan.chunks, max, &out.max_chunk);
    out.tag_diff = rowsum_noise(fresh_levels(plan.chunks.n_rows()), plan.diff, max, nullptr);
    return out;
}

GcmLongNoise aes_gcm_long_noise_schedule(const std::vector<NoiseLevel> &rk, const std::vector<NoiseLevel> &hk,
                                         const std::vector<NoiseLevel> &sk, size_t seg, const GcmFrame &f, int rounds,
                                         uint64_t max, int nr) {
    require_rounds(rounds, nr);
    require_gcm_rounds(rounds);
    require_key_words(rk.size(), nr, "expanded key");
    if (!f.m() || f.n_pub() < 2 || hk.size() % 128 || sk.size() % 128)
        throw ModelError{TAE_E_ARG, "empty GCM frame or a broken power table"};
    throw_gcm_long(gcm_long_shape_check(f.m(), seg, hk.size() / 128, sk.size() / 128));
    // every row before any level: the refusal does not depend on how far the replay got
    const size_t C = gcm_long_segments(f.m(), seg), table_blocks = std::min(seg, f.m());
    std::vector<std::vector<int32_t>> rows;
    std::vector<GcmInnerPlan> inner(C - 1);
    for (size_t c = 1; c < C; c++) {
        gcm_segment_rows(f, seg, c, 128, rows);
        if (!gcm_inner_rows_ok(rows)) throw_gcm_long(GCM_LONG_NOISE);
        gcm_inner_plan_add(inner[c - 1], rows);
    }
    gcm_long_final_rows(f, seg, table_blocks + 1, rows);
    if (!gcm_final_rows_ok(rows)) throw_gcm_long(GCM_LONG_NOISE);
    const std::vector<NoiseLevel> triv(128, NoiseLevel::trivial());
    GcmLongNoise out;
    out.plain.resize(f.data_len * 8);
    for (size_t b = 0; b * 16 < f.data_len; b++) {
        const std::vector<NoiseLevel> ks = aes_noise_schedule(rk, triv, rounds, max, nr);
        for (size_t i = 0; i < 128 && (b * 16 + i / 8) < f.data_len; i++) out.plain[b * 128 + i] = ks[i];
    }
    // the final source array of a one-frame call: the table's first blocks, E(J0), then the products
    std::vector<NoiseLevel> src(hk.begin(), hk.begin() + (std::ptrdiff_t)(table_blocks * 128));
    const std::vector<NoiseLevel> j0 = aes_noise_schedule(rk, triv, rounds, max, nr);
    src.insert(src.end(), j0.begin(), j0.end());
    const GcmProductPlan pp = gcm_product_plan();
    for (size_t c = 1; c < C; c++) {
        const GcmInnerPlan &ip = inner[c - 1];
        rowsum_noise(src, ip.chunks, max, &out.max_inner_chunk);  // reads table bits only: indices below 128 seg
        rowsum_noise(fresh_levels(ip.chunks.n_rows()), ip.rows, max, &out.max_inner_row);
        // S_c is refreshed to noise^2 = 1 with fresh ids; the product's partial bits are fresh whatever its operands
        const std::vector<NoiseLevel> prod = product_noise(pp, max, &out.max_part_chunk, &out.max_reduced);
        src.insert(src.end(), prod.begin(), prod.end());
    }
    GcmCallPlan plan;
    const std::vector<uint8_t> no_tag((size_t)f.tag_len, 0);
    gcm_call_plan_add(plan, rows, table_blocks, 0, no_tag.data());
    rowsum_noise(src, plan.chunks, max, &out.max_chunk);
    out.tag_diff = rowsum_noise(fresh_levels(plan.chunks.n_rows()), plan.diff, max, nullptr);
    return out;
}

namespace {
std::vector<GcmFrame> gcm_frames(const std::vector<Context::GcmFrameIn> &in, int tag_len) {
    std::vector<GcmFrame> frames(in.size());
    const size_t T = tag_len > 0 ? (size_t)tag_len : 0;
    for (size_t s = 0; s < in.size(); s++) {
        const Context::GcmFrameIn &st = in[s];
        if (!st.iv || (!st.aad && st.aad_len) || (!st.data && st.len)) throw ModelError{TAE_E_ARG, "null frame array"};
        switch (gcm_format(st.iv, st.iv_len, st.aad, st.aad_len, st.data, st.len >= T ? st.len - T : 0, tag_len, frames[s])) {
            case GCM_FMT_IV: throw ModelError{TAE_E_PARAM, "only 12-byte GCM IVs are supported"};
            case GCM_FMT_TAG: throw ModelError{TAE_E_PARAM, "a GCM tag is 4, 8 or 12 .. 16 bytes"};
            default: break;
        }
        if (st.len < T) throw ModelError{TAE_E_PARAM, "GCM data is shorter than the tag"};
    }
    return frames;
}
}  // namespace

// ---- the power tables: a single key is a table of one slot.  The forms keep their own argument
// checks; what follows them is shared ----
void Context::ghash_key_raw_call(const uint64_t *table, size_t n_keys, int n_powers, int rounds, int nr, size_t key_cts,
                                 uint64_t *out, bool device_mem) {
    // the single-key schedule: batching keys mixes no ciphertexts of different keys
    aes_ghash_key_noise_schedule(fresh_levels(key_cts), n_powers, rounds, params().max_noise_sq, nr);
    Staged st(*this, device_mem);
    engine_->ghash_key_multi(st.in(table, n_keys * key_cts * bit_len()), n_keys, n_powers, rounds, nr,
                             st.out(out, n_keys * (size_t)n_powers * 128 * bit_len()));
    st.finish();
}

std::vector<BitCt> Context::ghash_key_bits(const std::vector<const BitCt *> &table, size_t n_keys, int n_powers,
                                           int rounds, int nr, size_t kw) {
    const size_t L = bit_len();
    const std::vector<uint64_t> tab = gather_bits(table, L);
    std::vector<NoiseLevel> noise;  // the single-key bookkeeping, slot by slot
    for (size_t s = 0; s < n_keys; s++) {
        std::vector<NoiseLevel> krk(kw);
        for (size_t i = 0; i < kw; i++) krk[i] = table[s * kw + i]->noise;
        GhashKeyNoise kn = aes_ghash_key_noise_schedule(krk, n_powers, rounds, params().max_noise_sq, nr);
        for (NoiseLevel &x : kn.table) noise.push_back(std::move(x));
    }
    std::vector<uint64_t> hk(noise.size() * L);
    {
        Staged st(*this, false);
        engine_->ghash_key_multi(st.in(tab.data(), tab.size()), n_keys, n_powers, rounds, nr, st.out(hk.data(), hk.size()));
        st.finish();
    }
    return wrap_bits(hk, std::move(noise), L, params().max_noise_sq);
}

void Context::aes_ghash_key_raw(const uint64_t *rk, int n_powers, int rounds, uint64_t *out, bool device_mem, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    ghash_key_raw_call(rk, 1, n_powers, rounds, nr, (size_t)aes_words(key_bits) * 32, out, device_mem);
}

std::vector<BitCt> Context::aes_ghash_key(const std::vector<const BitCt *> &expanded_key, int n_powers, int rounds,
                                          int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    require_key_words(expanded_key.size(), nr, "expanded key");
    return ghash_key_bits(expanded_key, 1, n_powers, rounds, nr, (size_t)aes_words(key_bits) * 32);
}

void Context::aes_ghash_key_multi_raw(const uint64_t *table, size_t n_keys, int n_powers, int rounds, uint64_t *out,
                                      bool device_mem, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    require_powers(n_powers);
    if (!n_keys) return;
    if (!gcm_multi_shape_ok(n_keys, (size_t)n_powers, 0)) throw ModelError{TAE_E_PARAM, "at most 65536 keys a call"};
    ghash_key_raw_call(table, n_keys, n_powers, rounds, nr, (size_t)aes_words(key_bits) * 32, out, device_mem);
}

std::vector<BitCt> Context::aes_ghash_key_multi(const std::vector<const BitCt *> &table, size_t n_keys, int n_powers,
                                                int rounds, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    require_powers(n_powers);
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    if (table.size() != n_keys * kw) throw ModelError{TAE_E_ARG, "the key table is n_keys expanded keys"};
    if (!n_keys) return {};
    if (!gcm_multi_shape_ok(n_keys, (size_t)n_powers, 0)) throw ModelError{TAE_E_PARAM, "at most 65536 keys a call"};
    return ghash_key_bits(table, n_keys, n_powers, rounds, nr, kw);
}

// ---- frames of at most n_powers hashed blocks ----
namespace {
const uint8_t *data_of(const Context::GcmFrameIn &f) { return f.data; }
const uint8_t *data_of(const Context::GcmStreamIn &s) { return s.f.data; }

// The handle forms' assembly: replay(s) is the schedule of frame s, whose plain and tag_diff levels are appended in
// frame order; call(plain, tag_diff) fills the words; both results are wrapped
template <class Replay, class Call>
Context::GcmBits gcm_bits(size_t n_frames, size_t L, uint64_t max, Replay replay, Call call) {
    std::vector<NoiseLevel> pn, tn;
    for (size_t s = 0; s < n_frames; s++) {
        auto gn = replay(s);
        for (NoiseLevel &x : gn.plain) pn.push_back(std::move(x));
        for (NoiseLevel &x : gn.tag_diff) tn.push_back(std::move(x));
    }
    std::vector<uint64_t> plain(pn.size() * L), tag(tn.size() * L);
    call(plain.data(), tag.data());
    // xor with a public bit adds no noise
    return {wrap_bits(plain, std::move(pn), L, max), wrap_bits(tag, std::move(tn), L, max)};
}
}  // namespace

// what the engine's frame calls take: every frame with its ciphertext and its received tag, under slot 0 until
// gcm_call writes the staged slots; the u64 words of both outputs
template <class In>
Context::GcmStaging Context::gcm_staging(const std::vector<GcmFrame> &frames, const std::vector<In> &in,
                                         int tag_len) const {
    GcmStaging g;
    g.ein.resize(frames.size());
    for (size_t s = 0; s < frames.size(); s++) {
        g.ein[s] = {0, &frames[s], data_of(in[s]), data_of(in[s]) + frames[s].data_len};
        g.plain_words += frames[s].data_len * 8 * bit_len();
    }
    g.tag_words = frames.size() * 8 * (size_t)tag_len * bit_len();
    return g;
}

// The frames of a call through the engine; host memory uploads the named slots of both tables alone, renumbered alike.
// A single key is a table of one slot whose power table is not bounded by 64 (key_table = false)
void Context::gcm_call(const uint64_t *table, size_t n_keys, bool key_table, const uint64_t *htable, size_t n_powers,
                       std::vector<int32_t> slots, GcmStaging g, int rounds, int nr, size_t key_cts, uint64_t *out_plain,
                       uint64_t *out_tag_diff, bool device_mem) {
    const size_t S = bit_len();
    Staged st(*this, device_mem);
    std::vector<int32_t> hslots = slots;
    const uint64_t *d_tab = st.table(table, slots, key_cts * S), *d_htab = st.table(htable, hslots, n_powers * 128 * S);
    if (!device_mem) n_keys = (size_t)*std::max_element(slots.begin(), slots.end()) + 1;
    for (size_t s = 0; s < g.ein.size(); s++) g.ein[s].slot = slots[s];
    uint64_t *d_plain = st.out(out_plain, g.plain_words), *d_tag = st.out(out_tag_diff, g.tag_words);
    if (key_table)
        engine_->aes_gcm_transcipher_multi(d_tab, n_keys, d_htab, n_powers, g.ein, rounds, nr, d_plain, d_tag);
    else
        engine_->aes_gcm_transcipher(d_tab, d_htab, n_powers, g.ein, rounds, nr, d_plain, d_tag);
    st.finish();
}

void Context::aes_gcm_raw(const uint64_t *rk, const uint64_t *hk, size_t n_powers, const std::vector<GcmFrameIn> &in,
                          int tag_len, int rounds, uint64_t *out_plain, uint64_t *out_tag_diff, bool device_mem,
                          int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    require_gcm_rounds(rounds);
    if (!n_powers) throw ModelError{TAE_E_PARAM, "the power table is empty"};
    const std::vector<GcmFrame> frames = gcm_frames(in, tag_len);
    if (frames.empty()) return;
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    const std::vector<NoiseLevel> krk = fresh_levels(kw), khk = fresh_levels(n_powers * 128);
    for (const GcmFrame &f : frames) aes_gcm_noise_schedule(krk, khk, f, rounds, params().max_noise_sq, nr);
    gcm_call(rk, 1, false, hk, n_powers, std::vector<int32_t>(frames.size(), 0), gcm_staging(frames, in, tag_len), rounds,
             nr, kw, out_plain, out_tag_diff, device_mem);
}

Context::GcmBits Context::aes_gcm(const std::vector<const BitCt *> &expanded_key, const std::vector<const BitCt *> &hk,
                                  const std::vector<GcmFrameIn> &in, int tag_len, int rounds, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    require_gcm_rounds(rounds);
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    require_key_words(expanded_key.size(), nr, "expanded key");
    if (hk.empty() || hk.size() % 128) throw ModelError{TAE_E_ARG, "the power table is n_powers * 128 bits"};
    const size_t n_powers = hk.size() / 128;
    if (!n_powers) throw ModelError{TAE_E_PARAM, "the power table is empty"};
    const std::vector<GcmFrame> frames = gcm_frames(in, tag_len);
    if (frames.empty()) return {};
    std::vector<NoiseLevel> krk(kw), khk(hk.size());
    for (size_t i = 0; i < kw; i++) krk[i] = expanded_key[i]->noise;
    for (size_t i = 0; i < hk.size(); i++) khk[i] = hk[i]->noise;
    return gcm_bits(
        frames.size(), L, params().max_noise_sq,
        [&](size_t s) { return aes_gcm_noise_schedule(krk, khk, frames[s], rounds, params().max_noise_sq, nr); },
        [&](uint64_t *plain, uint64_t *tag) {
            const std::vector<uint64_t> rk = gather_bits(expanded_key, L), table = gather_bits(hk, L);
            gcm_call(rk.data(), 1, false, table.data(), n_powers, std::vector<int32_t>(frames.size(), 0),
                     gcm_staging(frames, in, tag_len), rounds, nr, kw, plain, tag, false);
        });
}

// ---- GCM over key tables ----
std::vector<GcmFrame> gcm_multi_frames(const std::vector<Context::GcmStreamIn> &in, size_t n_keys, size_t n_powers,
                                       int tag_len, std::vector<int32_t> &slots) {
    std::vector<Context::GcmFrameIn> fin(in.size());
    for (size_t s = 0; s < in.size(); s++) fin[s] = in[s].f;
    std::vector<GcmFrame> frames = gcm_frames(fin, tag_len);
    slots.resize(in.size());
    if (in.empty()) return frames;
    if (!gcm_multi_shape_ok(n_keys, n_powers, in.size()))
        throw ModelError{TAE_E_PARAM, "n_powers must be in 1..=64, and at most 65536 keys and 1048576 frames a call"};
    std::vector<std::vector<int32_t>> rows;
    for (size_t s = 0; s < in.size(); s++) {
        gcm_frame_rows(frames[s], rows);
        switch (gcm_multi_frame_check(frames[s], in[s].slot, n_keys, n_powers, tag_len, rows)) {
            case GCM_MULTI_SLOT: throw ModelError{TAE_E_ARG, "a frame's key slot is outside 0..n_keys-1"};
            case GCM_MULTI_POWERS:
                throw ModelError{TAE_E_PARAM, "the frame has more hashed blocks than the power table has powers"};
            case GCM_MULTI_NOISE: throw ModelError{TAE_E_NOISE, "a tag row needs more than 64 refreshed chunks"};
            case GCM_MULTI_TAG: throw ModelError{TAE_E_PARAM, "the frames of a call have one tag length"};
            default: break;
        }
        slots[s] = in[s].slot;
    }
    return frames;
}

void Context::aes_gcm_multi_raw(const uint64_t *table, size_t n_keys, const uint64_t *htable, size_t n_powers,
                                const std::vector<GcmStreamIn> &in, int tag_len, int rounds, uint64_t *out_plain,
                                uint64_t *out_tag_diff, bool device_mem, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    require_gcm_rounds(rounds);
    if (!n_powers) throw ModelError{TAE_E_PARAM, "the power table is empty"};
    std::vector<int32_t> slots;
    const std::vector<GcmFrame> frames = gcm_multi_frames(in, n_keys, n_powers, tag_len, slots);
    if (frames.empty()) return;
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    const std::vector<NoiseLevel> krk = fresh_levels(kw), khk = fresh_levels(n_powers * 128);
    for (const GcmFrame &f : frames) aes_gcm_noise_schedule(krk, khk, f, rounds, params().max_noise_sq, nr);
    gcm_call(table, n_keys, true, htable, n_powers, slots, gcm_staging(frames, in, tag_len), rounds, nr, kw, out_plain,
             out_tag_diff, device_mem);
}

Context::GcmBits Context::aes_gcm_multi(const BitAt &table, size_t n_keys, const BitAt &htable, size_t n_powers,
                                        const std::vector<GcmStreamIn> &in, int tag_len, int rounds, int key_bits) {
    const int nr = require_multi(key_bits, rounds);
    require_gcm_rounds(rounds);
    if (!n_powers) throw ModelError{TAE_E_PARAM, "the power table is empty"};
    std::vector<int32_t> slots;
    const std::vector<GcmFrame> frames = gcm_multi_frames(in, n_keys, n_powers, tag_len, slots);
    if (frames.empty()) return {};
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    std::vector<std::vector<NoiseLevel>> knoise, hnoise;
    std::vector<int32_t> hslots = slots;
    const std::vector<uint64_t> tab = gather_slots(table, slots, kw, L, knoise);
    const std::vector<uint64_t> htab = gather_slots(htable, hslots, n_powers * 128, L, hnoise);
    return gcm_bits(
        frames.size(), L, params().max_noise_sq,
        [&](size_t s) {
            return aes_gcm_noise_schedule(knoise[(size_t)slots[s]], hnoise[(size_t)slots[s]], frames[s], rounds,
                                          params().max_noise_sq, nr);
        },
        [&](uint64_t *plain, uint64_t *tag) {
            gcm_call(tab.data(), knoise.size(), true, htab.data(), n_powers, slots, gcm_staging(frames, in, tag_len),
                     rounds, nr, kw, plain, tag, false);
        });
}

// ---- frames beyond one table: segmented GHASH ----
void Context::aes_ghash_stride_key_raw(const uint64_t *hk, size_t n_powers, size_t seg, int n_strides, uint64_t *out,
                                       bool device_mem) {
    if (params().model != 1) throw ModelError{TAE_E_PARAM, "GCM runs on the 1-bit WoP-PBS parameter sets only"};
    if (!n_powers) throw ModelError{TAE_E_PARAM, "the power table is empty"};
    if (seg < 1 || seg > n_powers || seg > (size_t)kGcmMaxPowers)
        throw ModelError{TAE_E_PARAM, "seg must be in 1..=min(n_powers, 64)"};
    // the replay reads block seg - 1 alone: a fresh table of seg blocks stands for the caller's n_powers
    aes_ghash_stride_key_noise_schedule(fresh_levels(seg * 128), seg, n_strides, params().max_noise_sq);
    Staged st(*this, device_mem);
    engine_->ghash_stride_key(st.in(hk, n_powers * 128 * bit_len()), n_powers, seg, n_strides,
                              st.out(out, (size_t)n_strides * 128 * bit_len()));
    st.finish();
}

std::vector<BitCt> Context::aes_ghash_stride_key(const std::vector<const BitCt *> &hk, size_t seg, int n_strides) {
    if (params().model != 1) throw ModelError{TAE_E_PARAM, "GCM runs on the 1-bit WoP-PBS parameter sets only"};
    if (hk.empty() || hk.size() % 128) throw ModelError{TAE_E_ARG, "the power table is n_powers * 128 bits"};
    const size_t L = bit_len(), n_powers = hk.size() / 128;
    std::vector<NoiseLevel> khk(hk.size());
    for (size_t i = 0; i < hk.size(); i++) khk[i] = hk[i]->noise;
    GhashKeyNoise kn = aes_ghash_stride_key_noise_schedule(khk, seg, n_strides, params().max_noise_sq);
    const std::vector<uint64_t> table = gather_bits(hk, L);
    std::vector<uint64_t> sk(kn.table.size() * L);
    {
        Staged st(*this, false);
        engine_->ghash_stride_key(st.in(table.data(), table.size()), n_powers, seg, n_strides, st.out(sk.data(), sk.size()));
        st.finish();
    }
    return wrap_bits(sk, std::move(kn.table), L, params().max_noise_sq);
}

void Context::gcm_long_call(const uint64_t *rk, const uint64_t *hk, size_t n_powers, const uint64_t *sk, size_t n_strides,
                            size_t seg, const std::vector<GcmFrame> &frames, const std::vector<GcmFrameIn> &in,
                            int tag_len, int rounds, int nr, size_t key_cts, uint64_t *out_plain, uint64_t *out_tag_diff,
                            bool device_mem) {
    const size_t S = bit_len();
    const GcmStaging g = gcm_staging(frames, in, tag_len);
    Staged st(*this, device_mem);
    const uint64_t *d_rk = st.in(rk, key_cts * S), *d_hk = st.in(hk, n_powers * 128 * S);
    const uint64_t *d_sk = st.in(sk, n_strides * 128 * S);
    uint64_t *d_plain = st.out(out_plain, g.plain_words), *d_tag = st.out(out_tag_diff, g.tag_words);
    engine_->aes_gcm_long_transcipher(d_rk, d_hk, n_powers, d_sk, n_strides, seg, g.ein, rounds, nr, d_plain, d_tag);
    st.finish();
}

void Context::aes_gcm_long_raw(const uint64_t *rk, const uint64_t *hk, size_t n_powers, const uint64_t *sk,
                               size_t n_strides, size_t seg, const std::vector<GcmFrameIn> &in, int tag_len, int rounds,
                               uint64_t *out_plain, uint64_t *out_tag_diff, bool device_mem, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    require_gcm_rounds(rounds);
    if (!n_powers) throw ModelError{TAE_E_PARAM, "the power table is empty"};
    // before tables of that length are made for the replay
    throw_gcm_long(gcm_long_shape_check(1, seg, n_powers, n_strides));
    const std::vector<GcmFrame> frames = gcm_frames(in, tag_len);
    if (frames.empty()) return;
    const size_t kw = (size_t)aes_words(key_bits) * 32;
    // seg <= 64 and n_strides <= 64 by the shape check above: the replay's tables are bounded whatever n_powers is
    const std::vector<NoiseLevel> krk = fresh_levels(kw), khk = fresh_levels(seg * 128), ksk = fresh_levels(n_strides * 128);
    // the replay reads the table's first seg blocks only: hk stands for a table of n_powers through the shape check
    for (const GcmFrame &f : frames) {
        throw_gcm_long(gcm_long_shape_check(f.m(), seg, n_powers, n_strides));
        aes_gcm_long_noise_schedule(krk, khk, ksk, seg, f, rounds, params().max_noise_sq, nr);
    }
    gcm_long_call(rk, hk, n_powers, sk, n_strides, seg, frames, in, tag_len, rounds, nr, kw, out_plain, out_tag_diff,
                  device_mem);
}

Context::GcmBits Context::aes_gcm_long(const std::vector<const BitCt *> &expanded_key, const std::vector<const BitCt *> &hk,
                                       const std::vector<const BitCt *> &sk, size_t seg, const std::vector<GcmFrameIn> &in,
                                       int tag_len, int rounds, int key_bits) {
    const int nr = require_inverse(rounds, key_bits);
    require_gcm_rounds(rounds);
    const size_t kw = (size_t)aes_words(key_bits) * 32, L = bit_len();
    require_key_words(expanded_key.size(), nr, "expanded key");
    if (hk.empty() || hk.size() % 128 || sk.size() % 128)
        throw ModelError{TAE_E_ARG, "the power table and the stride key are n * 128 bits"};
    const size_t n_powers = hk.size() / 128, n_strides = sk.size() / 128;
    throw_gcm_long(gcm_long_shape_check(1, seg, n_powers, n_strides));
    const std::vector<GcmFrame> frames = gcm_frames(in, tag_len);
    if (frames.empty()) return {};
    // the stride key's levels are not consulted (model.hpp): its length alone goes into the replay
    const std::vector<NoiseLevel> ksk(sk.size());
    std::vector<NoiseLevel> krk(kw), khk(hk.size());
    for (size_t i = 0; i < kw; i++) krk[i] = expanded_key[i]->noise;
    for (size_t i = 0; i < hk.size(); i++) khk[i] = hk[i]->noise;
    return gcm_bits(
        frames.size(), L, params().max_noise_sq,
        [&](size_t s) {
            return aes_gcm_long_noise_schedule(krk, khk, ksk, seg, frames[s], rounds, params().max_noise_sq, nr);
        },
        [&](uint64_t *plain, uint64_t *tag) {
            const std::vector<uint64_t> rk = gather_bits(expanded_key, L), table = gather_bits(hk, L),
                                        strides = gather_bits(sk, L);
            gcm_long_call(rk.data(), table.data(), n_powers, strides.data(), n_strides, seg, frames, in, tag_len, rounds,
                          nr, kw, plain, tag, false);
        });
}

void Context::gf128_square_raw(const uint64_t *in, size_t count, uint64_t *out, bool device_mem) {
    if (params().model != 1) throw ModelError{TAE_E_PARAM, "GCM runs on the 1-bit WoP-PBS parameter sets only"};
    if (!count) return;
    const size_t len = count * 128 * bit_len();
    Staged st(*this, device_mem);
    engine_->gf128_square(st.in(in, len), count, st.out(out, len));
    st.finish();
}

void Context::gf128_product_raw(const uint64_t *a, const uint64_t *b, size_t count, uint64_t *out, bool device_mem) {
    if (params().model != 1) throw ModelError{TAE_E_PARAM, "GCM runs on the 1-bit WoP-PBS parameter sets only"};
    if (!count) return;
    const size_t len = count * 128 * bit_len();
    Staged st(*this, device_mem);
    engine_->gf128_product(st.in(a, len), st.in(b, len), count, st.out(out, len));
    st.finish();
}

// ---------------------------------------------------------------------------------------------
// AEAD open: the verdict bit and the verdict-gated payload (aead_open.hpp).  The reference has no AEAD.
// ---------------------------------------------------------------------------------------------
AeadOpenNoise aead_open_noise_schedule(const std::vector<NoiseLevel> &plain, const std::vector<NoiseLevel> &diff,
                                       const VerdictPlan &verdict, const GatePlan &gate, uint64_t max) {
    const size_t n = verdict.n_frames;
    if (verdict.levels() < 1 || diff.size() != n * verdict.bits[0] || gate.n_frames != n ||
        (!plain.empty() && plain.size() != gate.n_bytes() * 8))
        throw ModelError{TAE_E_ARG, "the bits do not match the plans"};
    // MaxNoiseLevel::validate on an input of a bootstrap
    auto input = [max](const NoiseLevel &x) {
        if (x.noise_level_squared > max)
            throw ModelError{TAE_E_NOISE, "NoiseTooBig { noise_level: " + std::to_string(x.noise_level_squared) +
                                              ", max_noise_level: " + std::to_string(max) + " }"};
    };
    auto outputs = [](size_t count, uint64_t level) {
        std::vector<NoiseLevel> o(count);
        for (auto &x : o) x = NoiseLevel::with_noise_level(level, next_ct_id());
        return o;
    };
    std::vector<NoiseLevel> cur = diff;
    for (int l = 0; l < verdict.levels(); l++) {
        for (int32_t s : verdict.idx[l])
            if (s >= 0) input(cur[(size_t)s]);  // the padding is the trivial zero
        cur = outputs(n * verdict.groups[l], kOpenOrBits);
    }
    AeadOpenNoise out;
    out.ok = std::move(cur);
    if (plain.empty()) return out;
    for (size_t g = 0; g < gate.n_bytes(); g++) {
        for (int b = 0; b < 8; b++) input(plain[g * 8 + b]);
        input(out.ok[(size_t)gate.frame_of_byte[g]]);
    }
    out.plain = outputs(plain.size(), kOpenGateBits);
    return out;
}

const Context::OpenLuts &Context::open_luts() {
    std::call_once(open_once_, [this] {
        const AeadOpenTables t = aead_open_tables();
        open_luts_.or8 = generate_lookup_table(kOpenOrBits, 1, t.or8.data());
        open_luts_.nor8 = generate_lookup_table(kOpenOrBits, 1, t.nor8.data());
        open_luts_.gate = generate_lookup_table(kOpenGateBits, 8, t.gate.data());
    });
    return open_luts_;
}

namespace {
void require_open(const Params &p, int tag_len) {
    if (p.model != 1) throw ModelError{TAE_E_PARAM, "the AEAD open runs on the 1-bit WoP-PBS parameter sets only"};
    if (!aead_tag_len_ok(tag_len)) throw ModelError{TAE_E_PARAM, "a tag is 4 .. 16 bytes, and even or 13 or 15"};
}
}  // namespace

// the verdicts, and with `gate` the gated payload, in one staging scope; the tables go up with the call
void Context::open_call(const uint64_t *plain, const GatePlan *gate, const uint64_t *tag_diff, const VerdictPlan &verdict,
                        uint64_t *out_plain, uint64_t *out_ok, bool device_mem) {
    const OpenLuts &luts = open_luts();
    const size_t n = verdict.n_frames, L = bit_len();
    std::vector<std::vector<int32_t>> gate_idx;
    if (gate)
        for (size_t g0 = 0, pass = engine_->aead_gate_pass(); g0 < gate->n_bytes(); g0 += pass)
            gate_idx.push_back(aead_gate_pass_index(*gate, g0, std::min(pass, gate->n_bytes() - g0)));
    Staged st(*this, device_mem);
    st.own_times();
    const uint64_t *d_diff = st.in(tag_diff, n * verdict.bits[0] * L);
    uint64_t *d_ok = st.out(out_ok, n * L);
    std::vector<const int32_t *> d_idx;
    for (const std::vector<int32_t> &ix : verdict.idx) d_idx.push_back(st.pub(ix.data(), ix.size()));
    engine_->aead_verdict(d_diff, verdict, d_idx, st.pub(luts.or8.data.data(), luts.or8.data.size()),
                          st.pub(luts.nor8.data.data(), luts.nor8.data.size()), d_ok);
    if (gate && gate->n_bytes()) {
        const size_t len = gate->n_bytes() * 8 * L;
        std::vector<const int32_t *> d_gidx;
        for (const std::vector<int32_t> &ix : gate_idx) d_gidx.push_back(st.pub(ix.data(), ix.size()));
        engine_->aead_gate(st.in(plain, len), *gate, d_gidx, d_ok, st.pub(luts.gate.data.data(), luts.gate.data.size()),
                           st.out(out_plain, len));
    }
    st.finish();
}

void Context::aead_verdict_raw(const uint64_t *tag_diff, size_t n_frames, int tag_len, uint64_t *ok, bool device_mem) {
    require_open(params(), tag_len);
    if (!n_frames) return;
    const VerdictPlan verdict = aead_verdict_plan(tag_len, n_frames);
    GatePlan none;
    none.n_frames = n_frames;
    const std::vector<NoiseLevel> at_cap(n_frames * verdict.bits[0], NoiseLevel{params().max_noise_sq, {}});
    aead_open_noise_schedule({}, at_cap, verdict, none, params().max_noise_sq);
    open_call(nullptr, nullptr, tag_diff, verdict, nullptr, ok, device_mem);
}

void Context::aead_open_raw(const uint64_t *plain, const size_t *payload_lens, const uint64_t *tag_diff, size_t n_frames,
                            int tag_len, uint64_t *out_plain, uint64_t *out_ok, bool device_mem) {
    require_open(params(), tag_len);
    if (!n_frames) return;
    const VerdictPlan verdict = aead_verdict_plan(tag_len, n_frames);
    const GatePlan gate = aead_gate_plan(payload_lens, n_frames);
    if (gate.n_bytes() && (!plain || !out_plain)) throw ModelError{TAE_E_ARG, "null"};
    const NoiseLevel cap{params().max_noise_sq, {}};
    aead_open_noise_schedule(std::vector<NoiseLevel>(gate.n_bytes() * 8, cap),
                             std::vector<NoiseLevel>(n_frames * verdict.bits[0], cap), verdict, gate, params().max_noise_sq);
    open_call(plain, &gate, tag_diff, verdict, out_plain, out_ok, device_mem);
}

Context::OpenBits Context::aead_open(const std::vector<const BitCt *> &plain, const size_t *payload_lens,
                                     const std::vector<const BitCt *> &tag_diff, size_t n_frames, int tag_len) {
    require_open(params(), tag_len);
    if (!n_frames) return {};
    const size_t L = bit_len();
    const VerdictPlan verdict = aead_verdict_plan(tag_len, n_frames);
    const GatePlan gate = aead_gate_plan(payload_lens, n_frames);
    if (plain.size() != gate.n_bytes() * 8 || tag_diff.size() != n_frames * verdict.bits[0])
        throw ModelError{TAE_E_ARG, "the bits do not match the payload lengths and the tag length"};
    std::vector<NoiseLevel> pn(plain.size()), dn(tag_diff.size());
    for (size_t i = 0; i < plain.size(); i++) pn[i] = plain[i]->noise;
    for (size_t i = 0; i < tag_diff.size(); i++) dn[i] = tag_diff[i]->noise;
    // a frame of no payload has no group, and a call of no payload no gate: the schedule then walks the verdict alone
    AeadOpenNoise on = aead_open_noise_schedule(pn, dn, verdict, gate, params().max_noise_sq);
    const std::vector<uint64_t> in = gather_bits(plain, L), diff = gather_bits(tag_diff, L);
    std::vector<uint64_t> out(in.size()), ok(n_frames * L);
    open_call(in.data(), &gate, diff.data(), verdict, out.data(), ok.data(), false);
    return {wrap_bits(out, std::move(on.plain), L, params().max_noise_sq),
            wrap_bits(ok, std::move(on.ok), L, params().max_noise_sq)};
}

// ---------------------------------------------------------------------------------------------
// shortint_1bit model (src/tfhe/shortint_1bit.rs)
// ---------------------------------------------------------------------------------------------
void Context::require_s1() const {
    if (params().model != 2) throw ModelError{TAE_E_PARAM, "this call belongs to the shortint_1bit parameter set"};
}

void Context::s1_bootstrap_raw(const uint64_t *in, size_t B, const uint64_t *tvs, size_t n_tv, uint64_t *out,
                               bool device_mem) {
    require_s1();
    if (n_tv < 1) throw ModelError{TAE_E_ARG, "at least one test vector"};
    const size_t L = bit_len(), G = params().glwe_len();
    Staged st(*this, device_mem);
    st.own_times();
    engine_->s1_bootstrap(st.in(in, B * L), st.pub(tvs, n_tv * G), n_tv, st.out(out, B * L), B);
    st.finish();
}

// ---- packed ciphertext I/O (glwe_pack.hpp) ----
void Context::require_pack(size_t count) const {
    if (params().id != SQRD_LVL_64)
        throw ModelError{TAE_E_PARAM, "packed ciphertext I/O is built for params_sqrd_lvl_64 only"};
    if (!count) throw ModelError{TAE_E_ARG, "a packed call needs at least one bit"};
}

void Context::unpack_bits_raw(const uint64_t *glwes, size_t count, uint64_t *bits, bool device_mem) {
    require_pack(count);
    const size_t G = glwe_pack::glwe_count(count, params().N);
    Staged st(*this, device_mem);
    st.own_times();
    engine_->unpack_bits(st.in(glwes, G * params().glwe_len()), count, st.out(bits, count * bit_len()));
    st.finish();
}

std::vector<BitCt> Context::unpack_bits(const uint64_t *glwes, size_t count) {
    require_pack(count);
    std::vector<uint64_t> raw(count * bit_len());
    unpack_bits_raw(glwes, count, raw.data(), false);
    std::vector<BitCt> out;
    out.reserve(count);
    for (size_t i = 0; i < count; i++)
        out.push_back(wrap(std::vector<uint64_t>(raw.begin() + i * bit_len(), raw.begin() + (i + 1) * bit_len()), 1));
    return out;
}

void Context::pack_bits_raw(const uint64_t *bits, size_t count, uint64_t *glwes, bool device_mem) {
    require_pack(count);
    const size_t G = glwe_pack::glwe_count(count, params().N);
    Staged st(*this, device_mem);
    engine_->pack_bits(st.in(bits, count * bit_len()), count, st.out(glwes, G * params().glwe_len()));
    st.finish();
}

void Context::pack_bits(const std::vector<const BitCt *> &bits, uint64_t *glwes) {
    require_pack(bits.size());
    const size_t L = bit_len();
    std::vector<uint64_t> raw(bits.size() * L);
    for (size_t i = 0; i < bits.size(); i++) {
        if (bits[i]->ct.size() != L) throw ModelError{TAE_E_ARG, "ciphertext size mismatch"};
        std::copy(bits[i]->ct.begin(), bits[i]->ct.end(), raw.begin() + i * L);
    }
    pack_bits_raw(raw.data(), bits.size(), glwes, false);
}

void Context::pack_pfks_raw(const uint64_t *bits, size_t count, uint64_t *glwes, bool device_mem) {
    require_pack(count);
    Staged st(*this, device_mem);
    st.own_times();
    engine_->pack_pfks(st.in(bits, count * bit_len()), count, st.out(glwes, count * params().glwe_len()));
    st.finish();
}

// ---- the engine's stages one at a time (tae_stage_*; no noise rule).  Host outputs are cleared first, as not every
// stage writes every word: pfks_into_ggsw fills only the rows of its level ----
void Context::keyswitch_raw(const uint64_t *in, size_t count, uint64_t *out, bool device_mem) {
    Staged st(*this, device_mem);
    st.own_times();
    engine_->keyswitch(st.in(in, count * params().big_len()), st.out_zeroed(out, count * params().small_len()), count);
    st.finish();
}

void Context::pbs_shift_boolean_raw(const uint64_t *small, size_t count, int level, uint64_t *big, bool device_mem) {
    Staged st(*this, device_mem);
    st.own_times();
    engine_->pbs_shift_boolean(st.in(small, count * params().small_len()), st.out_zeroed(big, count * params().big_len()),
                               count, level);
    st.finish();
}

void Context::bootstrap_raw(const uint64_t *small, size_t count, const uint64_t *lut_glwe, uint64_t *big,
                            bool device_mem) {
    Staged st(*this, device_mem);
    st.own_times();
    engine_->bootstrap(st.in(small, count * params().small_len()), st.lut(lut_glwe, params().glwe_len()),
                       st.out_zeroed(big, count * params().big_len()), count, 0, 0);
    st.finish();
}

void Context::pfks_ggsw_raw(const uint64_t *big, size_t count, int level, uint64_t *ggsw, bool device_mem) {
    Staged st(*this, device_mem);
    st.own_times();
    engine_->pfks_into_ggsw(st.in(big, count * params().big_len()), st.out_zeroed(ggsw, count * params().cbs_ggsw_len()),
                            count, level);
    st.finish();
}

void Context::ggsw_fourier_raw(const uint64_t *ggsw, size_t count, cplx *ggsw_f, bool device_mem) {
    Staged st(*this, device_mem);
    st.own_times();
    engine_->ggsw_to_fourier(st.in(ggsw, count * params().cbs_ggsw_len()),
                             st.out_zeroed(ggsw_f, count * params().cbs_ggsw_fourier_len()), count);
    st.finish();
}

void Context::vertical_packing_raw(const cplx *ggsw_f, size_t groups, int n_in, const uint64_t *lut, int n_out,
                                   uint64_t *out, bool device_mem) {
    int log_n = 0;
    while ((1 << log_n) < params().N) log_n++;
    // n_in > log2 N: the LUT of every output holds 2^tree polynomials (the CMux tree's leaves)
    const int tree = std::max(0, n_in - log_n);
    if (tree > 16) throw ModelError{TAE_E_ARG, "n_in exceeds log2 N + 16"};
    Staged st(*this, device_mem);
    st.own_times();
    engine_->vertical_packing(st.in(ggsw_f, groups * n_in * params().cbs_ggsw_fourier_len()), groups, n_in,
                              st.lut(lut, (size_t)n_out * ((size_t)params().N << tree)), n_out,
                              st.out_zeroed(out, groups * n_out * params().big_len()));
    st.finish();
}

// lhs += rhs over count ciphertexts (tae_xor_batch, after its noise rule)
void Context::xor_raw(uint64_t *lhs, const uint64_t *rhs, size_t count, bool device_mem) {
    if (!count) return;
    const size_t words = count * bit_len();
    Staged st(*this, device_mem);
    engine_->lwe_add(st.inout(lhs, words), st.in(rhs, words), words);
    st.finish();
}

void Context::s1_packing_keyswitch_raw(const uint64_t *cts, size_t count, uint64_t *glwe, bool device_mem) {
    require_s1();
    if (count < 1 || count > (size_t)params().N) throw ModelError{TAE_E_ARG, "packing keyswitch takes 1..N ciphertexts"};
    Staged st(*this, device_mem);
    st.own_times();
    engine_->s1_pack(st.in(cts, count * bit_len()), (int)count, st.out(glwe, params().glwe_len()));
    st.finish();
}

void Context::s1_test_vectors_from_ciphertexts_raw(const uint64_t *ct0, const uint64_t *ct1, size_t B, uint64_t *tvs,
                                                   bool device_mem) {
    require_s1();
    const size_t L = bit_len(), G = params().glwe_len();
    std::lock_guard<std::mutex> g(mu_);
    hip_check(hipSetDevice(engine_->device()), "hipSetDevice");
    // interleave the pairs (2b, 2b+1) = (ct0[b], ct1[b]) on the device, as the tree levels hold them
    DevBuf<uint64_t> d_pairs(2 * B * L), d_pks(2 * B * G);
    const auto kind = device_mem ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (device_mem) engine_->order_after_caller();
    hip_check(hipMemcpy2DAsync(d_pairs, 2 * L * 8, ct0, L * 8, L * 8, B, kind, engine_->stream()), "pairs");
    hip_check(hipMemcpy2DAsync(d_pairs + L, 2 * L * 8, ct1, L * 8, L * 8, B, kind, engine_->stream()),
              "pairs");
    engine_->begin_call();
    engine_->s1_pks(d_pairs, 2 * B, d_pks);
    if (device_mem) {
        engine_->s1_tv_from_pks(d_pks, B, tvs);
    } else {
        DevBuf<uint64_t> d_tv(B * G);
        engine_->s1_tv_from_pks(d_pks, B, d_tv);
        hip_check(hipMemcpyAsync(tvs, d_tv, B * G * 8, hipMemcpyDeviceToHost, engine_->stream()), "download");
        engine_->synchronize();
        return;
    }
    engine_->synchronize();
}

void Context::s1_multivariate_raw(const uint64_t *bits, size_t G, int nbits, const uint64_t *f_tables, int n_fn,
                                  uint64_t *out, bool device_mem) {
    require_s1();
    if (nbits < 1 || nbits > 8) throw ModelError{TAE_E_ARG, "multivariate functions take 1..=8 bits (shortint_1bit.rs:526)"};
    if (n_fn < 1) throw ModelError{TAE_E_ARG, "at least one function"};
    const size_t L = bit_len(), GL = params().glwe_len(), V = (size_t)1 << (nbits - 1);
    // generate_multivariate_test_vector (:519-536): test vector v of function f selects f(2v + bit)
    std::vector<uint64_t> tvs((size_t)n_fn * V * GL);
    for (int f = 0; f < n_fn; f++)
        for (size_t v = 0; v < V; v++) {
            const uint64_t *tab = f_tables + (size_t)f * 2 * V;
            if (tab[2 * v] > 1 || tab[2 * v + 1] > 1) throw ModelError{TAE_E_ARG, "function values must be 0 or 1"};
            s1_test_vector(params(), tab[2 * v], tab[2 * v + 1], &tvs[((size_t)f * V + v) * GL]);
        }
    Staged st(*this, device_mem);
    st.own_times();
    engine_->s1_multivariate(st.in(bits, G * nbits * L), G, nbits, st.pub(tvs.data(), tvs.size()), n_fn,
                             st.out(out, G * n_fn * L));
    st.finish();
}

}  // namespace tae
