// extern "C" boundary (include/tfhe_aes_gpu.h).  Each entry point maps a reference trait method
// or tfhe-rs call to the host model (model.cpp) and the device Engine (kernels.hip); panics of the
// reference become status codes, HIP failures TAE_E_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../include/tfhe_aes_gpu.h"
#include "aes.hpp"
#include "client.hpp"
#include "engine.hpp"
#include "glwe_pack.hpp"
#include "cplx.hpp"
#include "model.hpp"

struct tae_client_key {
    tae::ClientKey ck;
};
struct tae_context {
    std::unique_ptr<tae::Context> ctx;
};
struct tae_bit {
    tae::BitCt b;
};
struct tae_lut {
    tae::Lut l;
};

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

template <class F>
int guarded(F &&fn) {
    try {
        fn();
        return TAE_OK;
    } catch (const tae::ModelError &e) {
        return fail(e.code, e.msg);
    } catch (const tae::HipError &e) {
        return fail(TAE_E_HIP, e.msg);
    } catch (const std::bad_alloc &) {
        return fail(TAE_E_ARG, "out of host memory");
    } catch (const std::exception &e) {
        return fail(TAE_E_PARAM, e.what());
    }
}

void require(bool cond, const char *msg) {
    if (!cond) throw tae::ModelError{TAE_E_ARG, msg};
}

tae::Params params_of(int param_set) {
    tae::Params p;
    if (!tae::get_params(param_set, p)) throw tae::ModelError{TAE_E_PARAM, "unknown parameter set"};
    return p;
}

void fill(tae_params *o, const tae::Params &p) {
    *o = {p.n, p.k, p.N, p.pbs_l, p.pbs_b, p.ks_l, p.ks_b, p.cbs_l, p.cbs_b, p.pfks_l, p.pfks_b,
          p.lwe_std, p.glwe_std, p.pfks_std, p.max_noise_sq, p.model};
}

void require_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        throw tae::ModelError{TAE_E_NODEV, "no GPU available: the HIP path has no CPU fallback"};
    if (device < 0 || device >= count) throw tae::ModelError{TAE_E_NODEV, "device index out of range"};
}

std::vector<const tae::BitCt *> unwrap(const tae_bit *const *bits, size_t n) {
    std::vector<const tae::BitCt *> v(n);
    for (size_t i = 0; i < n; i++) {
        require(bits[i] != nullptr, "null bit handle");
        v[i] = &bits[i]->b;
    }
    return v;
}

void emit(const std::vector<tae::BitCt> &res, tae_bit **out) {
    for (size_t i = 0; i < res.size(); i++) out[i] = new tae_bit{res[i]};
}

}  // namespace

extern "C" {

const char *tae_last_error(void) { return g_last_error.c_str(); }
const char *tae_version(void) { return "tfhe-aes-2_amd 0.1 (gfx950)"; }

int tae_device_count(int *count) {
    return guarded([&] {
        require(count, "null");
        *count = 0;
        if (hipGetDeviceCount(count) != hipSuccess) *count = 0;
    });
}

int tae_get_params(int param_set, tae_params *out) {
    return guarded([&] {
        require(out, "null");
        fill(out, params_of(param_set));
    });
}

int tae_bit_len(int param_set, size_t *len) {
    return guarded([&] {
        require(len, "null");
        const tae::Params p = params_of(param_set);
        *len = p.bit_len();
    });
}

int tae_server_key_sizes(int param_set, size_t *ksk_len, size_t *bsk_len, size_t *pfpksk_len) {
    return guarded([&] {
        const tae::Params p = params_of(param_set);
        if (ksk_len) *ksk_len = p.ksk_len();
        if (bsk_len) *bsk_len = p.bsk_len();
        if (pfpksk_len) *pfpksk_len = p.pfpksk_len();
    });
}

int tae_generate_keys_raw(int param_set, const uint8_t seed[32], int threads, tae_client_key **client_key,
                          uint64_t *ksk, uint64_t *bsk, uint64_t *pfpksk) {
    return guarded([&] {
        require(seed && client_key, "null argument");
        const tae::Params p = params_of(param_set);
        auto ck = std::make_unique<tae_client_key>();
        tae::ServerKeyRaw sk;
        tae::generate_keys(p, seed, threads, ck->ck, sk);
        if (ksk) std::memcpy(ksk, sk.ksk.data(), sk.ksk.size() * 8);
        if (bsk) std::memcpy(bsk, sk.bsk.data(), sk.bsk.size() * 8);
        if (pfpksk) std::memcpy(pfpksk, sk.pfpksk.data(), sk.pfpksk.size() * 8);
        *client_key = ck.release();
    });
}

int tae_generate_keys(int param_set, const uint8_t seed[32], int device, int threads, tae_client_key **client_key,
                      tae_context **context) {
    return guarded([&] {
        require(seed && client_key && context, "null argument");
        const tae::Params p = params_of(param_set);
        require_device(device);
        auto ck = std::make_unique<tae_client_key>();
        tae::ServerKeyRaw sk;
        tae::generate_keys(p, seed, threads, ck->ck, sk);
        auto ctx = std::make_unique<tae_context>();
        ctx->ctx = std::make_unique<tae::Context>(std::make_unique<tae::Engine>(sk, device));
        *client_key = ck.release();
        *context = ctx.release();
    });
}

int tae_client_key_from_seed(int param_set, const uint8_t seed[32], tae_client_key **client_key) {
    return guarded([&] {
        require(seed && client_key, "null argument");
        auto ck = std::make_unique<tae_client_key>();
        tae::generate_client_key(params_of(param_set), seed, ck->ck);
        *client_key = ck.release();
    });
}

extern "C++" {
namespace tae {
namespace keyio {
void save(const char *path, const Params &p, int param_set, const ClientKey *ck, const uint64_t *ksk,
          const uint64_t *bsk, const uint64_t *pfpksk);
void load(const char *path, int *param_set, uint32_t *flags, ClientKey *ck, uint64_t *ksk, uint64_t *bsk,
          uint64_t *pfpksk);
}  // namespace keyio
}  // namespace tae
}

int tae_keys_save(const char *path, int param_set, const tae_client_key *client_key, const uint64_t *ksk,
                  const uint64_t *bsk, const uint64_t *pfpksk) {
    return guarded([&] {
        require(path, "null path");
        const tae::Params p = params_of(param_set);
        if (client_key) {
            const tae::Params &q = client_key->ck.p;
            require(q.n == p.n && q.k == p.k && q.N == p.N && q.model == p.model,
                    "client key does not belong to the parameter set");
        }
        tae::keyio::save(path, p, param_set, client_key ? &client_key->ck : nullptr, ksk, bsk, pfpksk);
    });
}

int tae_keys_file_info(const char *path, int *param_set, int *flags) {
    return guarded([&] {
        require(path && param_set && flags, "null argument");
        uint32_t fl = 0;
        tae::keyio::load(path, param_set, &fl, nullptr, nullptr, nullptr, nullptr);
        *flags = (int)fl;
    });
}

int tae_keys_load(const char *path, tae_client_key **client_key, uint64_t *ksk, uint64_t *bsk, uint64_t *pfpksk) {
    return guarded([&] {
        require(path, "null path");
        require(client_key || ksk || bsk || pfpksk, "nothing to load");
        int ps = 0;
        uint32_t fl = 0;
        std::unique_ptr<tae_client_key> ck = client_key ? std::make_unique<tae_client_key>() : nullptr;
        tae::keyio::load(path, &ps, &fl, ck ? &ck->ck : nullptr, ksk, bsk, pfpksk);
        if (client_key) *client_key = ck.release();
    });
}

int tae_context_create_raw(int param_set, int device, const uint64_t *ksk, const uint64_t *bsk,
                           const uint64_t *pfpksk, int mem, tae_context **context) {
    return guarded([&] {
        require(ksk && bsk && pfpksk && context, "null argument");
        const tae::Params p = params_of(param_set);
        require_device(device);
        auto ctx = std::make_unique<tae_context>();
        if (mem == TAE_MEM_DEVICE) {
            ctx->ctx = std::make_unique<tae::Context>(std::make_unique<tae::Engine>(p, device, ksk, bsk, pfpksk));
        } else {
            tae::ServerKeyRaw sk;
            sk.p = p;
            sk.ksk.assign(ksk, ksk + p.ksk_len());
            sk.bsk.assign(bsk, bsk + p.bsk_len());
            sk.pfpksk.assign(pfpksk, pfpksk + p.pfpksk_len());
            ctx->ctx = std::make_unique<tae::Context>(std::make_unique<tae::Engine>(sk, device));
        }
        *context = ctx.release();
    });
}

void tae_context_free(tae_context *ctx) { delete ctx; }
void tae_client_key_free(tae_client_key *ck) { delete ck; }

int tae_client_key_secrets(const tae_client_key *ck, uint64_t *lwe_sk, uint64_t *glwe_sk) {
    return guarded([&] {
        require(ck, "null");
        if (lwe_sk) std::memcpy(lwe_sk, ck->ck.lwe_sk.data(), ck->ck.lwe_sk.size() * 8);
        if (glwe_sk) std::memcpy(glwe_sk, ck->ck.glwe_sk.data(), ck->ck.glwe_sk.size() * 8);
    });
}

int tae_context_params(const tae_context *ctx, tae_params *out) {
    return guarded([&] {
        require(ctx && out, "null");
        fill(out, ctx->ctx->params());
    });
}

int tae_encrypt(const tae_client_key *ck, uint64_t bit, tae_bit **out) {
    return guarded([&] {
        require(ck && out, "null");
        if (bit > 1) throw tae::ModelError{TAE_E_ARG, "cleartext out of bounds: " + std::to_string(bit)};
        auto &c = const_cast<tae_client_key *>(ck)->ck;
        auto b = std::make_unique<tae_bit>();
        b->b.ct.assign(c.bit_len(), 0);
        c.encrypt_model_bit_at(bit, tae::kAutoIndexBase + c.next_index.fetch_add(1), b->b.ct.data());
        // BitCt::fresh (1-bit model: noise^2 1 + a new component id; 8-bit: NoiseLevel::NOMINAL)
        b->b.noise = c.p.model == 8   ? tae::NoiseLevel{1, {}}
                     : c.p.model == 2 ? tae::NoiseLevel{}  // shortint_1bit: unchecked adds, nothing tracked
                                      : tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        b->b.max_noise_sq = c.p.max_noise_sq;
        *out = b.release();
    });
}

int tae_decrypt(const tae_client_key *ck, const tae_bit *bit, uint64_t *out) {
    return guarded([&] {
        require(ck && bit && out, "null");
        require(bit->b.ct.size() == ck->ck.bit_len(), "ciphertext size mismatch");
        *out = ck->ck.decrypt_model_bit(bit->b.ct.data());
    });
}

int tae_trivial(const tae_context *ctx, uint64_t bit, tae_bit **out) {
    return guarded([&] {
        require(ctx && out, "null");
        *out = new tae_bit{ctx->ctx->trivial(bit)};
    });
}

// Resolve the encryption indices of a raw call: TAE_INDEX_AUTO reserves `count` fresh indices from
// the key's counter (the region tae_encrypt uses); an explicit range must lie below kAutoIndexBase.
static uint64_t raw_index_range(const tae_client_key *ck, size_t count, uint64_t start_index) {
    if (start_index == TAE_INDEX_AUTO) return tae::kAutoIndexBase + const_cast<tae_client_key *>(ck)->ck.next_index.fetch_add(count);
    require(start_index < tae::kAutoIndexBase && count <= tae::kAutoIndexBase - start_index,
            "explicit encryption indices must lie below 2^63 (use TAE_INDEX_AUTO for fresh ones)");
    return start_index;
}

int tae_encrypt_bits_raw(const tae_client_key *ck, const uint8_t *bits, size_t count, uint64_t start_index,
                         uint64_t *out) {
    return guarded([&] {
        require(ck && (bits || !count) && (out || !count), "null");
        for (size_t i = 0; i < count; i++) require(bits[i] < 2, "cleartext out of bounds");
        const uint64_t first = raw_index_range(ck, count, start_index);
        const size_t L = ck->ck.bit_len();
        for (size_t i = 0; i < count; i++) ck->ck.encrypt_model_bit_at(bits[i], first + i, out + i * L);
    });
}

int tae_encrypt_ints_raw(const tae_client_key *ck, const uint8_t *values, size_t count, uint64_t start_index,
                         uint64_t *out) {
    return guarded([&] {
        require(ck && (values || !count) && (out || !count), "null");
        const uint64_t first = raw_index_range(ck, count, start_index);
        const size_t L = ck->ck.p.big_len();
        for (size_t i = 0; i < count; i++) ck->ck.encrypt_int_at(values[i], first + i, out + i * L);
    });
}

int tae_decrypt_ints_raw(const tae_client_key *ck, const uint64_t *cts, size_t count, uint8_t *values) {
    return guarded([&] {
        require(ck && (cts || !count) && (values || !count), "null");
        const size_t L = ck->ck.p.big_len();
        for (size_t i = 0; i < count; i++) values[i] = (uint8_t)ck->ck.decrypt_int(cts + i * L);
    });
}

int tae_decrypt_bits_raw(const tae_client_key *ck, const uint64_t *cts, size_t count, uint8_t *bits) {
    return guarded([&] {
        require(ck && (cts || !count) && (bits || !count), "null");
        const size_t L = ck->ck.bit_len();
        for (size_t i = 0; i < count; i++) bits[i] = (uint8_t)ck->ck.decrypt_model_bit(cts + i * L);
    });
}

int tae_bit_clone(const tae_bit *bit, tae_bit **out) {
    return guarded([&] {
        require(bit && out, "null");
        *out = new tae_bit{bit->b};
    });
}

void tae_bit_free(tae_bit *bit) { delete bit; }

int tae_bit_xor_assign(tae_bit *lhs, const tae_bit *rhs) {
    return guarded([&] {
        require(lhs && rhs, "null");
        lhs->b.xor_assign(rhs->b);
    });
}

int tae_bit_noise_level(const tae_bit *bit, uint64_t *nl) {
    return guarded([&] {
        require(bit && nl, "null");
        *nl = bit->b.noise.noise_level_squared;
    });
}

int tae_bit_data(const tae_bit *bit, uint64_t *out, size_t len) {
    return guarded([&] {
        require(bit && out, "null");
        require(len == bit->b.ct.size(), "length mismatch");
        std::memcpy(out, bit->b.ct.data(), len * 8);
    });
}

int tae_bit_from_data(const tae_context *ctx, const uint64_t *data, size_t len, uint64_t nl, tae_bit **out) {
    return guarded([&] {
        require(ctx && data && out, "null");
        require(len == ctx->ctx->bit_len(), "length mismatch");
        *out = new tae_bit{ctx->ctx->wrap(std::vector<uint64_t>(data, data + len), nl)};
    });
}

int tae_generate_lookup_table(const tae_context *ctx, int input_bits, int output_bits, const uint64_t *f_values,
                              tae_lut **out) {
    return guarded([&] {
        require(ctx && f_values && out, "null");
        *out = new tae_lut{ctx->ctx->generate_lookup_table(input_bits, output_bits, f_values)};
    });
}

void tae_lut_free(tae_lut *lut) { delete lut; }

int tae_generate_multivariate_luts(int poly_size, int input_bits, int output_bits, const uint64_t *f_values,
                                   uint64_t *out, size_t out_len) {
    return guarded([&] {
        require(f_values && out, "null");
        require(poly_size >= 2 && (poly_size & (poly_size - 1)) == 0 && poly_size <= (1 << 16),
                "polynomial size must be a power of two");
        require(input_bits >= 1 && input_bits <= 16 && output_bits >= 1 && output_bits <= 64, "bit counts out of range");
        require(out_len == tae::lut_small_len(poly_size, input_bits) * (size_t)output_bits, "length mismatch");
        tae::generate_lut(poly_size, input_bits, output_bits, f_values, out);
    });
}

int tae_xor_batch(const tae_context *ctx, uint64_t *lhs, const uint64_t *rhs, size_t count,
                  const uint64_t *lhs_noise_sq, const uint64_t *rhs_noise_sq, uint64_t *out_noise_sq, int mem) {
    return guarded([&] {
        require(ctx && (lhs || !count) && (rhs || !count), "null");
        require((lhs_noise_sq == nullptr) == (rhs_noise_sq == nullptr), "give both noise arrays or neither");
        const uint64_t max_sq = ctx->ctx->params().max_noise_sq;
        if (lhs_noise_sq) {
            // BitXorAssign's noise rule (shortint_woppbs_1bit.rs:134-142, NoiseLevelWithComponents::add
            // + MaxNoiseLevel::validate): squared noise levels add and must stay <= max_noise_level^2
            for (size_t i = 0; i < count; i++) {
                const uint64_t l = lhs_noise_sq[i], r = rhs_noise_sq[i];
                const uint64_t s = l + r;
                if (l > max_sq || r > max_sq - l)  // no wrap-around: l + r <= max_sq exactly
                    throw tae::ModelError{TAE_E_NOISE, "NoiseTooBig: noise level squared " + std::to_string(s) +
                                                           " above " + std::to_string(max_sq) + " at element " +
                                                           std::to_string(i)};
            }
        }
        ctx->ctx->xor_raw(lhs, rhs, count, mem == TAE_MEM_DEVICE);
        if (out_noise_sq && lhs_noise_sq)
            for (size_t i = 0; i < count; i++) out_noise_sq[i] = lhs_noise_sq[i] + rhs_noise_sq[i];
    });
}

int tae_lut_data(const tae_lut *lut, uint64_t *out, size_t len, size_t *needed) {
    return guarded([&] {
        require(lut, "null");
        if (needed) *needed = lut->l.data.size();
        if (out) {
            require(len == lut->l.data.size(), "length mismatch");
            std::memcpy(out, lut->l.data.data(), len * 8);
        }
    });
}

int tae_circuit_bootstrap(const tae_context *ctx, const tae_bit *const *bits, size_t n_bits, const tae_lut *lut,
                          tae_bit **out) {
    return guarded([&] {
        require(ctx && bits && lut && out, "null");
        emit(ctx->ctx->circuit_bootstrap(unwrap(bits, n_bits), lut->l), out);
    });
}

int tae_circuit_bootstrap_raw(const tae_context *ctx, const uint64_t *bits, size_t groups, int n_in,
                              const tae_lut *lut, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && bits && lut && out, "null");
        ctx->ctx->circuit_bootstrap_raw(bits, groups, n_in, lut->l, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_bootstrap_from_bits_raw(const tae_context *ctx, const uint64_t *bits, size_t groups, const tae_lut *lut,
                                uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && bits && lut && out, "null");
        ctx->ctx->bootstrap_from_bits_raw(bits, groups, lut->l, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_extract_bits_raw(const tae_context *ctx, const uint64_t *ints, size_t groups, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && ints && out, "null");
        ctx->ctx->extract_bits_raw(ints, groups, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_aes_key_schedule_raw(const tae_context *ctx, const uint64_t *key, uint64_t *expanded, int mem) {
    return guarded([&] {
        require(ctx && key && expanded, "null");
        ctx->ctx->aes_key_schedule_raw(key, expanded, mem == TAE_MEM_DEVICE);
    });
}

int tae_aes_encrypt_block_for_rounds(const tae_context *ctx, const tae_bit *const *expanded_key,
                                     const tae_bit *const *block, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx && expanded_key && block && out, "null");
        emit(ctx->ctx->aes_encrypt_blocks(unwrap(expanded_key, 44 * 32), unwrap(block, 128), 1, rounds), out);
    });
}

int tae_aes_encrypt_blocks(const tae_context *ctx, const tae_bit *const *expanded_key, const tae_bit *const *blocks,
                           size_t n_blocks, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx && expanded_key && blocks && out, "null");
        emit(ctx->ctx->aes_encrypt_blocks(unwrap(expanded_key, 44 * 32), unwrap(blocks, 128 * n_blocks), n_blocks,
                                          rounds),
             out);
    });
}

int tae_aes_key_schedule(const tae_context *ctx, const tae_bit *const *key, tae_bit **expanded) {
    return guarded([&] {
        require(ctx && key && expanded, "null");
        emit(ctx->ctx->aes_key_schedule(unwrap(key, 128)), expanded);
    });
}

int tae_aes_encrypt_blocks_raw(const tae_context *ctx, const uint64_t *rk, const uint64_t *blocks, size_t n_blocks,
                               int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && rk && blocks && out, "null");
        ctx->ctx->aes_encrypt_blocks_raw(rk, blocks, n_blocks, rounds, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_aes_ctr_plan(const uint8_t iv[8], uint64_t first_counter, size_t n_blocks, size_t *round1_groups) {
    return guarded([&] {
        require(iv && round1_groups, "null");
        tae::CtrPlan plan;
        if (!tae::ctr_plan(iv, first_counter, n_blocks, plan))
            throw tae::ModelError{TAE_E_ARG, "counter range wraps past 2^64 - 1"};
        *round1_groups = plan.groups.size();
    });
}

int tae_aes_ctr_keystream_raw(const tae_context *ctx, const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter,
                              size_t n_blocks, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && rk && iv && (out || !n_blocks), "null");
        ctx->ctx->aes_ctr_keystream_raw(rk, iv, first_counter, n_blocks, rounds, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_aes_ctr_transcipher_raw(const tae_context *ctx, const uint64_t *rk, const uint8_t iv[8], uint64_t first_counter,
                                const uint8_t *data, size_t len, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && rk && iv && ((data && out) || !len), "null");
        ctx->ctx->aes_ctr_transcipher_raw(rk, iv, first_counter, data, len, tae::kAesRounds, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_aes_ctr_transcipher(const tae_context *ctx, const tae_bit *const *expanded_key, const uint8_t iv[8],
                            uint64_t first_counter, const uint8_t *data, size_t len, tae_bit **out) {
    return guarded([&] {
        require(ctx && expanded_key && iv && ((data && out) || !len), "null");
        emit(ctx->ctx->aes_ctr_transcipher(unwrap(expanded_key, 44 * 32), iv, first_counter, data, len), out);
    });
}

/* ---- inverse cipher, FIPS-197 5.3 (no counterpart in the reference) ---- */
int tae_aes_decrypt_key(const tae_context *ctx, const tae_bit *const *expanded_key, tae_bit **dk) {
    return guarded([&] {
        require(ctx && expanded_key && dk, "null");
        emit(ctx->ctx->aes_decrypt_key(unwrap(expanded_key, 44 * 32)), dk);
    });
}

int tae_aes_decrypt_key_raw(const tae_context *ctx, const uint64_t *rk, uint64_t *dk, int mem) {
    return guarded([&] {
        require(ctx && rk && dk, "null");
        ctx->ctx->aes_decrypt_key_raw(rk, dk, mem == TAE_MEM_DEVICE);
    });
}

int tae_aes_decrypt_blocks(const tae_context *ctx, const tae_bit *const *dk, const tae_bit *const *blocks,
                           size_t n_blocks, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx && dk && (n_blocks == 0 || (blocks && out)), "null");
        emit(ctx->ctx->aes_decrypt_blocks(unwrap(dk, 44 * 32), unwrap(blocks, 128 * n_blocks), n_blocks, rounds), out);
    });
}

int tae_aes_decrypt_blocks_raw(const tae_context *ctx, const uint64_t *dk, const uint64_t *blocks, size_t n_blocks,
                               int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && dk && (n_blocks == 0 || (blocks && out)), "null");
        ctx->ctx->aes_decrypt_blocks_raw(dk, blocks, n_blocks, rounds, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_aes_cbc_transcipher(const tae_context *ctx, const tae_bit *const *dk, const uint8_t iv[16], const uint8_t *data,
                            size_t len, tae_bit **out) {
    return guarded([&] {
        require(ctx && dk && iv && ((data && out) || !len), "null");
        emit(ctx->ctx->aes_cbc_transcipher(unwrap(dk, 44 * 32), iv, data, len), out);
    });
}

int tae_aes_cbc_transcipher_raw(const tae_context *ctx, const uint64_t *dk, const uint8_t iv[16], const uint8_t *data,
                                size_t len, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && dk && iv && ((data && out) || !len), "null");
        ctx->ctx->aes_cbc_transcipher_raw(dk, iv, data, len, tae::kAesRounds, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_aes_decrypt_noise_schedule_check(int param_set, int rounds) {
    return guarded([&] {
        const tae::Params p = params_of(param_set);
        if (p.model != 1)
            throw tae::ModelError{TAE_E_PARAM, "the inverse cipher runs on the 1-bit WoP-PBS parameter sets only"};
        if (rounds < 1 || rounds > 10) throw tae::ModelError{TAE_E_PARAM, "rounds must be in 1..=10"};
        std::vector<tae::NoiseLevel> rk(44 * 32), blk(128);
        for (auto &x : rk) x = tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        for (auto &x : blk) x = tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        const std::vector<tae::NoiseLevel> dk = tae::aes_decrypt_key_noise_schedule(rk, p.max_noise_sq);
        tae::aes_decrypt_noise_schedule(dk, blk, rounds, p.max_noise_sq);
    });
}

/* ---- AES-128 / 192 / 256 by key_bits (FIPS-197 5.2 and figure 11; no counterpart in the reference) ---- */
namespace {
// ciphertexts of an expanded key; key_bits is checked before any handle array is read at that length
size_t key_cts(int key_bits) {
    if (!tae::aes_key_bits_ok(key_bits)) throw tae::ModelError{TAE_E_PARAM, "key_bits must be 128, 192 or 256"};
    return (size_t)tae::aes_words(key_bits) * 32;
}
constexpr tae::AesDriver kGalMul = tae::AesDriver::GalMul;
}  // namespace

int tae_aesx_expanded_words(int key_bits, size_t *words) {
    return guarded([&] {
        require(words != nullptr, "null");
        *words = key_cts(key_bits) / 32;
    });
}

int tae_aesx_key_schedule(const tae_context *ctx, int key_bits, const tae_bit *const *key, tae_bit **expanded) {
    return guarded([&] {
        require(ctx && key && expanded, "null");
        key_cts(key_bits);
        emit(ctx->ctx->aes_key_expand(unwrap(key, (size_t)key_bits), key_bits), expanded);
    });
}

int tae_aesx_key_schedule_raw(const tae_context *ctx, int key_bits, const uint64_t *key, uint64_t *expanded, int mem) {
    return guarded([&] {
        require(ctx && key && expanded, "null");
        ctx->ctx->aes_key_expand_raw(key, expanded, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_encrypt_blocks(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                            const tae_bit *const *blocks, size_t n_blocks, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx && expanded_key && blocks && out, "null");
        emit(ctx->ctx->aes_encrypt_blocks(unwrap(expanded_key, key_cts(key_bits)), unwrap(blocks, 128 * n_blocks),
                                          n_blocks, rounds, kGalMul, key_bits),
             out);
    });
}

int tae_aesx_encrypt_blocks_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint64_t *blocks,
                                size_t n_blocks, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && rk && blocks && out, "null");
        ctx->ctx->aes_encrypt_blocks_raw(rk, blocks, n_blocks, rounds, out, mem == TAE_MEM_DEVICE, kGalMul, key_bits);
    });
}

int tae_aesx_ctr_keystream_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint8_t iv[8],
                               uint64_t first_counter, size_t n_blocks, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && rk && iv && (out || !n_blocks), "null");
        ctx->ctx->aes_ctr_keystream_raw(rk, iv, first_counter, n_blocks, rounds, out, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_ctr_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint8_t iv[8],
                                 uint64_t first_counter, const uint8_t *data, size_t len, int rounds, uint64_t *out,
                                 int mem) {
    return guarded([&] {
        require(ctx && rk && iv && ((data && out) || !len), "null");
        ctx->ctx->aes_ctr_transcipher_raw(rk, iv, first_counter, data, len, rounds, out, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_ctr_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                             const uint8_t iv[8], uint64_t first_counter, const uint8_t *data, size_t len, int rounds,
                             tae_bit **out) {
    return guarded([&] {
        require(ctx && expanded_key && iv && ((data && out) || !len), "null");
        emit(ctx->ctx->aes_ctr_transcipher(unwrap(expanded_key, key_cts(key_bits)), iv, first_counter, data, len, rounds,
                                           key_bits),
             out);
    });
}

int tae_aesx_decrypt_key(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key, tae_bit **dk) {
    return guarded([&] {
        require(ctx && expanded_key && dk, "null");
        emit(ctx->ctx->aes_decrypt_key(unwrap(expanded_key, key_cts(key_bits)), key_bits), dk);
    });
}

int tae_aesx_decrypt_key_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, uint64_t *dk, int mem) {
    return guarded([&] {
        require(ctx && rk && dk, "null");
        ctx->ctx->aes_decrypt_key_raw(rk, dk, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_decrypt_blocks(const tae_context *ctx, int key_bits, const tae_bit *const *dk, const tae_bit *const *blocks,
                            size_t n_blocks, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx && dk && (n_blocks == 0 || (blocks && out)), "null");
        emit(ctx->ctx->aes_decrypt_blocks(unwrap(dk, key_cts(key_bits)), unwrap(blocks, 128 * n_blocks), n_blocks, rounds,
                                          key_bits),
             out);
    });
}

int tae_aesx_decrypt_blocks_raw(const tae_context *ctx, int key_bits, const uint64_t *dk, const uint64_t *blocks,
                                size_t n_blocks, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && dk && (n_blocks == 0 || (blocks && out)), "null");
        ctx->ctx->aes_decrypt_blocks_raw(dk, blocks, n_blocks, rounds, out, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_cbc_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *dk, const uint8_t iv[16],
                             const uint8_t *data, size_t len, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx && dk && iv && ((data && out) || !len), "null");
        emit(ctx->ctx->aes_cbc_transcipher(unwrap(dk, key_cts(key_bits)), iv, data, len, rounds, key_bits), out);
    });
}

int tae_aesx_cbc_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *dk, const uint8_t iv[16],
                                 const uint8_t *data, size_t len, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && dk && iv && ((data && out) || !len), "null");
        ctx->ctx->aes_cbc_transcipher_raw(dk, iv, data, len, rounds, out, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_noise_schedule_check(int param_set, int key_bits, int rounds, int inverse) {
    return guarded([&] {
        const tae::Params p = params_of(param_set);
        const size_t kw = key_cts(key_bits);
        const int nk = tae::aes_nk(key_bits), nr = tae::aes_nr(key_bits);
        if (p.model != 1)
            throw tae::ModelError{TAE_E_PARAM, "AES by key_bits runs on the 1-bit WoP-PBS parameter sets only"};
        if (rounds < 1 || rounds > nr)
            throw tae::ModelError{TAE_E_PARAM, "rounds must be in 1..=" + std::to_string(nr)};
        std::vector<tae::NoiseLevel> key((size_t)nk * 32), blk(128);
        for (auto &x : key) x = tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        for (auto &x : blk) x = tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        const std::vector<tae::NoiseLevel> rk = tae::aes_key_expand_noise_schedule(key, nk, p.max_noise_sq);
        require(rk.size() == kw, "expanded key size");
        if (inverse)
            tae::aes_decrypt_noise_schedule(tae::aes_decrypt_key_noise_schedule(rk, p.max_noise_sq, nr), blk, rounds,
                                            p.max_noise_sq, nr);
        else
            tae::aes_noise_schedule(rk, blk, rounds, p.max_noise_sq, nr);
    });
}

/* ---- XTS-AES decryption of a public ciphertext (IEEE 1619; no counterpart in the reference) ---- */
extern "C++" {
namespace {
// A compute call: the arguments first, then the device (a machine without one has no context to pass)
void require_xts_server(const tae_context *ctx) {
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0)
        throw tae::ModelError{TAE_E_NODEV, "no GPU available: the HIP path has no CPU fallback"};
    require(ctx != nullptr, "null");
}

std::vector<tae::Context::XtsUnitIn> xts_units_in(const tae_xts_unit *units, size_t n_units) {
    require(units || !n_units, "null");
    std::vector<tae::Context::XtsUnitIn> v(n_units);
    for (size_t i = 0; i < n_units; i++) {
        if (!units[i].len || units[i].len % 16)
            throw tae::ModelError{TAE_E_PARAM, "an XTS data unit is a positive number of whole 16-byte blocks"};
        require(units[i].data != nullptr, "null unit data");
        std::memcpy(v[i].tweak, units[i].tweak, 16);
        v[i].first_block = units[i].first_block;
        v[i].data = units[i].data;
        v[i].len = units[i].len;
    }
    return v;
}

// the 1-bit WoP-PBS sets, key_bits and rounds of an XTS check that has no context
tae::Params xts_params(int param_set, int key_bits, int rounds) {
    const tae::Params p = params_of(param_set);
    key_cts(key_bits);
    if (p.model != 1) throw tae::ModelError{TAE_E_PARAM, "XTS runs on the 1-bit WoP-PBS parameter sets only"};
    if (rounds < 1 || rounds > tae::aes_nr(key_bits))
        throw tae::ModelError{TAE_E_PARAM, "rounds must be in 1..=" + std::to_string(tae::aes_nr(key_bits))};
    return p;
}
}  // namespace
}  // extern "C++"

int tae_aesx_xts_row_weight(uint64_t block_index, int *weight) {
    return guarded([&] {
        require(weight != nullptr, "null");
        *weight = tae::xts_row_weight(block_index);
    });
}

int tae_aesx_xts_noise_schedule_check(int param_set, int key_bits, int rounds, uint64_t max_block_index) {
    return guarded([&] {
        const tae::Params p = xts_params(param_set, key_bits, rounds);
        const int nk = tae::aes_nk(key_bits), nr = tae::aes_nr(key_bits);
        auto fresh = [](size_t n) {
            std::vector<tae::NoiseLevel> v(n);
            for (auto &x : v) x = tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
            return v;
        };
        // both keys from fresh key bits: the two expansions, the decryption key of the first, the tweak, the block
        const std::vector<tae::NoiseLevel> rk1 = tae::aes_key_expand_noise_schedule(fresh((size_t)nk * 32), nk, p.max_noise_sq);
        const std::vector<tae::NoiseLevel> rk2 = tae::aes_key_expand_noise_schedule(fresh((size_t)nk * 32), nk, p.max_noise_sq);
        const std::vector<tae::NoiseLevel> dk1 = tae::aes_decrypt_key_noise_schedule(rk1, p.max_noise_sq, nr);
        const std::vector<tae::NoiseLevel> tweak = tae::aes_xts_tweak_noise_schedule(rk2, rounds, p.max_noise_sq, nr);
        tae::aes_xts_noise_schedule(dk1, tweak, max_block_index, rounds, p.max_noise_sq, nr);
    });
}

int tae_aesx_xts_tweaks_raw(const tae_context *ctx, int key_bits, const uint64_t *rk2, const uint8_t *tweaks, size_t n,
                            int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(rk2 && ((tweaks && out) || !n), "null");
        key_cts(key_bits);
        require_xts_server(ctx);
        ctx->ctx->aes_xts_tweaks_raw(rk2, tweaks, n, rounds, out, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_stage_xts_masks(const tae_context *ctx, const uint64_t *tweaks_ct, size_t n_units, const int32_t *unit_of_block,
                        const uint64_t *block_index, size_t nb, uint64_t *masks, int mem) {
    return guarded([&] {
        require((tweaks_ct && unit_of_block && block_index && masks) || !nb, "null");
        require_xts_server(ctx);
        ctx->ctx->xts_masks_raw(tweaks_ct, n_units, unit_of_block, block_index, nb, masks, mem == TAE_MEM_DEVICE);
    });
}

int tae_aesx_xts_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *dk1, const uint64_t *rk2,
                                 const tae_xts_unit *units, size_t n_units, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(dk1 && rk2 && (out || !n_units), "null");
        key_cts(key_bits);
        const std::vector<tae::Context::XtsUnitIn> in = xts_units_in(units, n_units);
        require_xts_server(ctx);
        ctx->ctx->aes_xts_transcipher_raw(dk1, rk2, in, rounds, out, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_xts_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *dk1, const tae_bit *const *ek2,
                             const tae_xts_unit *units, size_t n_units, int rounds, tae_bit **out) {
    return guarded([&] {
        require(dk1 && ek2 && (out || !n_units), "null");
        const size_t kw = key_cts(key_bits);
        const std::vector<tae::Context::XtsUnitIn> in = xts_units_in(units, n_units);
        require_xts_server(ctx);
        emit(ctx->ctx->aes_xts_transcipher(unwrap(dk1, kw), unwrap(ek2, kw), in, rounds, key_bits), out);
    });
}

/* ---- multi-key batches: key tables [n_keys][W*32][L] (no counterpart in the reference) ---- */
extern "C++" {
namespace {
std::vector<tae::Context::CtrStreamIn> ctr_streams_in(const tae_ctr_stream *streams, size_t n_streams) {
    require(streams || !n_streams, "null");
    std::vector<tae::Context::CtrStreamIn> v(n_streams);
    for (size_t i = 0; i < n_streams; i++) {
        v[i].s.slot = streams[i].key;
        std::memcpy(v[i].s.iv, streams[i].iv, 8);
        v[i].s.first_counter = streams[i].first_counter;
        v[i].s.len = streams[i].len;
        v[i].data = streams[i].data;
    }
    return v;
}

std::vector<tae::Context::CbcStreamIn> cbc_streams_in(const tae_cbc_stream *streams, size_t n_streams) {
    require(streams || !n_streams, "null");
    std::vector<tae::Context::CbcStreamIn> v(n_streams);
    for (size_t i = 0; i < n_streams; i++) {
        require(streams[i].data || !streams[i].len, "null stream data");
        v[i].slot = streams[i].key;
        std::memcpy(v[i].iv, streams[i].iv, 16);
        v[i].data = streams[i].data;
        v[i].len = streams[i].len;
    }
    return v;
}

tae::Context::BitAt bit_at(const tae_bit *const *bits) {
    return [bits](size_t i) {
        require(bits[i] != nullptr, "null bit handle");
        return &bits[i]->b;
    };
}
}  // namespace
}  // extern "C++"

int tae_aesm_key_schedule_raw(const tae_context *ctx, int key_bits, const uint64_t *keys, size_t n_keys, uint64_t *table,
                              int mem) {
    return guarded([&] {
        require(ctx && ((keys && table) || !n_keys), "null");
        ctx->ctx->aes_key_expand_multi_raw(keys, n_keys, table, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_decrypt_key_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys, uint64_t *dtable,
                             int mem) {
    return guarded([&] {
        require(ctx && ((table && dtable) || !n_keys), "null");
        ctx->ctx->aes_decrypt_key_multi_raw(table, n_keys, dtable, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_encrypt_blocks_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                                const int32_t *key_of_block, const uint64_t *blocks, size_t n_blocks, int rounds,
                                uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && ((table && key_of_block && blocks && out) || !n_blocks), "null");
        ctx->ctx->aes_blocks_multi_raw(false, table, n_keys, key_of_block, blocks, n_blocks, rounds, out,
                                       mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_decrypt_blocks_raw(const tae_context *ctx, int key_bits, const uint64_t *dtable, size_t n_keys,
                                const int32_t *key_of_block, const uint64_t *blocks, size_t n_blocks, int rounds,
                                uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && ((dtable && key_of_block && blocks && out) || !n_blocks), "null");
        ctx->ctx->aes_blocks_multi_raw(true, dtable, n_keys, key_of_block, blocks, n_blocks, rounds, out,
                                       mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_ctr_plan(const tae_ctr_stream *streams, size_t n_streams, size_t *round1_groups) {
    return guarded([&] {
        require(round1_groups != nullptr, "null");
        const std::vector<tae::Context::CtrStreamIn> in = ctr_streams_in(streams, n_streams);
        std::vector<tae::CtrStream> ss(in.size());
        for (size_t i = 0; i < in.size(); i++) ss[i] = in[i].s;
        std::vector<tae::CtrBlock> blocks;
        switch (tae::ctr_flatten(ss.data(), ss.size(), -1, blocks)) {
            case tae::CTR_FLAT_SLOT: throw tae::ModelError{TAE_E_ARG, "a stream's key slot is negative"};
            case tae::CTR_FLAT_WRAP: throw tae::ModelError{TAE_E_ARG, "counter range wraps past 2^64 - 1"};
            default: break;
        }
        tae::CtrPlanMulti plan;
        tae::ctr_plan_multi(blocks.data(), blocks.size(), plan);
        *round1_groups = plan.groups.size();
    });
}

int tae_aesm_ctr_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                                 const tae_ctr_stream *streams, size_t n_streams, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx != nullptr, "null");
        const std::vector<tae::Context::CtrStreamIn> in = ctr_streams_in(streams, n_streams);
        size_t total = 0;
        for (const auto &s : in) total += s.s.len;
        require((table && out) || !total, "null");
        ctx->ctx->aes_ctr_multi_raw(table, n_keys, in, rounds, out, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_cbc_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *dtable, size_t n_keys,
                                 const tae_cbc_stream *streams, size_t n_streams, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx != nullptr, "null");
        const std::vector<tae::Context::CbcStreamIn> in = cbc_streams_in(streams, n_streams);
        size_t total = 0;
        for (const auto &s : in) total += s.len;
        require((dtable && out) || !total, "null");
        ctx->ctx->aes_cbc_multi_raw(dtable, n_keys, in, rounds, out, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_key_schedule(const tae_context *ctx, int key_bits, const tae_bit *const *keys, size_t n_keys,
                          tae_bit **table) {
    return guarded([&] {
        require(ctx && ((keys && table) || !n_keys), "null");
        key_cts(key_bits);  // key_bits is checked before the handle array is read at that length
        emit(ctx->ctx->aes_key_expand_multi(unwrap(keys, n_keys * (size_t)key_bits), n_keys, key_bits), table);
    });
}

int tae_aesm_ctr_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *table, size_t n_keys,
                             const tae_ctr_stream *streams, size_t n_streams, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx != nullptr, "null");
        const std::vector<tae::Context::CtrStreamIn> in = ctr_streams_in(streams, n_streams);
        size_t total = 0;
        for (const auto &s : in) total += s.s.len;
        require((table && out) || !total, "null");
        emit(ctx->ctx->aes_ctr_multi(bit_at(table), n_keys, in, rounds, key_bits), out);
    });
}

int tae_aesm_cbc_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *dtable, size_t n_keys,
                             const tae_cbc_stream *streams, size_t n_streams, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx != nullptr, "null");
        const std::vector<tae::Context::CbcStreamIn> in = cbc_streams_in(streams, n_streams);
        size_t total = 0;
        for (const auto &s : in) total += s.len;
        require((dtable && out) || !total, "null");
        emit(ctx->ctx->aes_cbc_multi(bit_at(dtable), n_keys, in, rounds, key_bits), out);
    });
}

/* ---- AES-CCM decryption of public frames (RFC 3610; no counterpart in the reference) ---- */
extern "C++" {
namespace {
std::vector<tae::Context::CcmStreamIn> ccm_streams_in(const tae_ccm_stream *streams, size_t n_streams) {
    require(streams || !n_streams, "null");
    std::vector<tae::Context::CcmStreamIn> v(n_streams);
    for (size_t i = 0; i < n_streams; i++)
        v[i] = {streams[i].key,  streams[i].nonce, streams[i].nonce_len, streams[i].aad,
                streams[i].aad_len, streams[i].data,  streams[i].len};
    return v;
}

void throw_ccm_format(tae::CcmFormat e) {
    switch (e) {
        case tae::CCM_FMT_NONCE: throw tae::ModelError{TAE_E_PARAM, "a CCM nonce is 7..13 bytes"};
        case tae::CCM_FMT_TAG: throw tae::ModelError{TAE_E_PARAM, "a CCM tag is 4, 6 .. 16 bytes"};
        case tae::CCM_FMT_AAD:
            throw tae::ModelError{TAE_E_PARAM, "CCM associated data of 0xFF00 bytes or more is not supported"};
        case tae::CCM_FMT_LEN:
            throw tae::ModelError{TAE_E_PARAM, "the payload length does not fit the nonce's length field"};
        default: break;
    }
}
}  // namespace
}  // extern "C++"

int tae_aesx_ccm_format(const uint8_t *nonce, size_t nonce_len, int tag_len, const uint8_t *aad, size_t aad_len,
                        size_t payload_len, size_t *n_ctr, size_t *n_mac, uint8_t *ctr_blocks, uint8_t *mac_blocks,
                        int64_t *mac_src) {
    return guarded([&] {
        require(nonce && n_ctr && n_mac && (aad || !aad_len), "null");
        tae::CcmFrame f;
        throw_ccm_format(tae::ccm_format(nonce, nonce_len, tag_len, aad, aad_len, payload_len, f));
        *n_ctr = f.n_ctr();
        *n_mac = f.n_mac();
        if (ctr_blocks) std::memcpy(ctr_blocks, f.ctr.data(), f.ctr.size());
        if (mac_blocks) std::memcpy(mac_blocks, f.mac.data(), f.mac.size());
        if (mac_src) std::memcpy(mac_src, f.src.data(), f.src.size() * sizeof(int64_t));
    });
}

int tae_aesx_ccm_noise_schedule_check(int param_set, int key_bits, int rounds) {
    return guarded([&] {
        const tae::Params p = params_of(param_set);
        const size_t kw = key_cts(key_bits);
        const int nk = tae::aes_nk(key_bits), nr = tae::aes_nr(key_bits);
        if (p.model != 1) throw tae::ModelError{TAE_E_PARAM, "CCM runs on the 1-bit WoP-PBS parameter sets only"};
        std::vector<tae::NoiseLevel> key((size_t)nk * 32);
        for (auto &x : key) x = tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        const std::vector<tae::NoiseLevel> rk = tae::aes_key_expand_noise_schedule(key, nk, p.max_noise_sq);
        require(rk.size() == kw, "expanded key size");
        // a frame with every kind of step: public AAD bytes, payload bytes and a padded last block
        const uint8_t nonce[13] = {}, aad[8] = {};
        tae::CcmFrame f;
        throw_ccm_format(tae::ccm_format(nonce, sizeof(nonce), 16, aad, sizeof(aad), 17, f));
        tae::aes_ccm_noise_schedule(rk, f, rounds, p.max_noise_sq, nr);
    });
}

int tae_aesm_pub_keystream_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                               const int32_t *key_of_block, const uint8_t *blocks, size_t n_blocks, int rounds,
                               uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && ((table && key_of_block && blocks && out) || !n_blocks), "null");
        ctx->ctx->aes_pub_keystream_multi_raw(table, n_keys, key_of_block, blocks, n_blocks, rounds, out,
                                              mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_ccm_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                                 const tae_ccm_stream *streams, size_t n_streams, int tag_len, int rounds,
                                 uint64_t *out_plain, uint64_t *out_tag_diff, int mem) {
    return guarded([&] {
        require(ctx != nullptr, "null");
        const std::vector<tae::Context::CcmStreamIn> in = ccm_streams_in(streams, n_streams);
        require((table && out_tag_diff) || !n_streams, "null");
        ctx->ctx->aes_ccm_multi_raw(table, n_keys, in, tag_len, rounds, out_plain, out_tag_diff, mem == TAE_MEM_DEVICE,
                                    key_bits);
    });
}

int tae_aesm_ccm_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *table, size_t n_keys,
                             const tae_ccm_stream *streams, size_t n_streams, int tag_len, int rounds,
                             tae_bit **out_plain, tae_bit **out_tag_diff) {
    return guarded([&] {
        require(ctx != nullptr, "null");
        const std::vector<tae::Context::CcmStreamIn> in = ccm_streams_in(streams, n_streams);
        require((table && out_tag_diff) || !n_streams, "null");
        const tae::Context::CcmBits res = ctx->ctx->aes_ccm_multi(bit_at(table), n_keys, in, tag_len, rounds, key_bits);
        require(out_plain || res.plain.empty(), "null");
        emit(res.plain, out_plain);
        emit(res.tag_diff, out_tag_diff);
    });
}

int tae_aesx_ccm_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint8_t *nonce,
                                 size_t nonce_len, const uint8_t *aad, size_t aad_len, const uint8_t *data, size_t len,
                                 int tag_len, int rounds, uint64_t *out_plain, uint64_t *out_tag_diff, int mem) {
    return guarded([&] {
        require(ctx && rk && out_tag_diff, "null");
        const std::vector<tae::Context::CcmStreamIn> in = {{0, nonce, nonce_len, aad, aad_len, data, len}};
        ctx->ctx->aes_ccm_multi_raw(rk, 1, in, tag_len, rounds, out_plain, out_tag_diff, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_ccm_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                             const uint8_t *nonce, size_t nonce_len, const uint8_t *aad, size_t aad_len,
                             const uint8_t *data, size_t len, int tag_len, int rounds, tae_bit **out_plain,
                             tae_bit **out_tag_diff) {
    return guarded([&] {
        require(ctx && expanded_key && out_tag_diff, "null");
        const std::vector<tae::Context::CcmStreamIn> in = {{0, nonce, nonce_len, aad, aad_len, data, len}};
        const tae::Context::CcmBits res = ctx->ctx->aes_ccm_multi(bit_at(expanded_key), 1, in, tag_len, rounds, key_bits);
        require(out_plain || res.plain.empty(), "null");
        emit(res.plain, out_plain);
        emit(res.tag_diff, out_tag_diff);
    });
}

/* ---- AES-GCM decryption of public frames (SP 800-38D; no counterpart in the reference) ---- */
extern "C++" {
namespace {
std::vector<tae::Context::GcmFrameIn> gcm_frames_in(const tae_gcm_frame *frames, size_t n_frames) {
    require(frames || !n_frames, "null");
    std::vector<tae::Context::GcmFrameIn> v(n_frames);
    for (size_t i = 0; i < n_frames; i++)
        v[i] = {frames[i].iv, frames[i].iv_len, frames[i].aad, frames[i].aad_len, frames[i].data, frames[i].len};
    return v;
}

void throw_gcm_format(tae::GcmFormat e) {
    if (e == tae::GCM_FMT_IV) throw tae::ModelError{TAE_E_PARAM, "only 12-byte GCM IVs are supported"};
    if (e == tae::GCM_FMT_TAG) throw tae::ModelError{TAE_E_PARAM, "a GCM tag is 4, 8 or 12 .. 16 bytes"};
}
}  // namespace
}  // extern "C++"

int tae_aesx_gcm_format(const uint8_t *iv, size_t iv_len, const uint8_t *aad, size_t aad_len, const uint8_t *data,
                        size_t data_len, int tag_len, size_t *n_pub, size_t *n_hashed, uint8_t *pub_blocks,
                        uint8_t *hashed_blocks) {
    return guarded([&] {
        require(iv && n_pub && n_hashed && (aad || !aad_len) && (data || !data_len), "null");
        tae::GcmFrame f;
        throw_gcm_format(tae::gcm_format(iv, iv_len, aad, aad_len, data, data_len, tag_len, f));
        *n_pub = f.n_pub();
        *n_hashed = f.m();
        if (pub_blocks) std::memcpy(pub_blocks, f.pub.data(), f.pub.size());
        if (hashed_blocks) std::memcpy(hashed_blocks, f.hashed.data(), f.hashed.size());
    });
}

int tae_aesx_gcm_tag_rows(const uint8_t *iv, size_t iv_len, const uint8_t *aad, size_t aad_len, const uint8_t *data,
                          size_t data_len, int tag_len, size_t n_powers, int32_t *row_sources, int32_t *row_chunks) {
    return guarded([&] {
        require(iv && row_sources && row_chunks && (aad || !aad_len) && (data || !data_len), "null");
        tae::GcmFrame f;
        throw_gcm_format(tae::gcm_format(iv, iv_len, aad, aad_len, data, data_len, tag_len, f));
        std::vector<std::vector<int32_t>> rows;
        tae::gcm_frame_rows(f, rows);
        for (size_t r = 0; r < rows.size(); r++) {
            row_sources[r] = (int32_t)rows[r].size();
            row_chunks[r] = (int32_t)tae::gcm_row_chunks(rows[r].size());
        }
        switch (tae::gcm_frame_check(f, n_powers, rows)) {
            case tae::GCM_PLAN_POWERS:
                throw tae::ModelError{TAE_E_PARAM, "the frame has more hashed blocks than the power table has powers"};
            case tae::GCM_PLAN_NOISE: throw tae::ModelError{TAE_E_NOISE, "a tag row needs more than 64 refreshed chunks"};
            default: break;
        }
    });
}

int tae_aesx_gcm_noise_schedule_check(int param_set, int key_bits, int rounds, int n_powers, size_t aad_len,
                                      size_t data_len) {
    return guarded([&] {
        const tae::Params p = params_of(param_set);
        const size_t kw = key_cts(key_bits);
        const int nk = tae::aes_nk(key_bits), nr = tae::aes_nr(key_bits);
        if (p.model != 1) throw tae::ModelError{TAE_E_PARAM, "GCM runs on the 1-bit WoP-PBS parameter sets only"};
        std::vector<tae::NoiseLevel> key((size_t)nk * 32);
        for (auto &x : key) x = tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        const std::vector<tae::NoiseLevel> rk = tae::aes_key_expand_noise_schedule(key, nk, p.max_noise_sq);
        require(rk.size() == kw, "expanded key size");
        const tae::GhashKeyNoise hk = tae::aes_ghash_key_noise_schedule(rk, n_powers, rounds, p.max_noise_sq, nr);
        // a frame of the given sizes with dense blocks: every byte 0xA5
        const uint8_t iv[12] = {};
        const std::vector<uint8_t> aad(aad_len, 0xA5), data(data_len, 0xA5);
        tae::GcmFrame f;
        throw_gcm_format(tae::gcm_format(iv, 12, aad.data(), aad_len, data.data(), data_len, 16, f));
        tae::aes_gcm_noise_schedule(rk, hk.table, f, rounds, p.max_noise_sq, nr);
    });
}

int tae_aesx_ghash_key_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, int n_powers, int rounds,
                           uint64_t *hk, int mem) {
    return guarded([&] {
        require(rk && hk, "null");
        key_cts(key_bits);
        require_xts_server(ctx);
        ctx->ctx->aes_ghash_key_raw(rk, n_powers, rounds, hk, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_ghash_key(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key, int n_powers, int rounds,
                       tae_bit **hk) {
    return guarded([&] {
        require(expanded_key && hk, "null");
        const size_t kw = key_cts(key_bits);
        require_xts_server(ctx);
        emit(ctx->ctx->aes_ghash_key(unwrap(expanded_key, kw), n_powers, rounds, key_bits), hk);
    });
}

int tae_aesx_gcm_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint64_t *hk,
                                 size_t n_powers, const tae_gcm_frame *frames, size_t n_frames, int tag_len, int rounds,
                                 uint64_t *out_plain, uint64_t *out_tag_diff, int mem) {
    return guarded([&] {
        require((rk && hk && out_tag_diff) || !n_frames, "null");
        key_cts(key_bits);
        const std::vector<tae::Context::GcmFrameIn> in = gcm_frames_in(frames, n_frames);
        require_xts_server(ctx);
        ctx->ctx->aes_gcm_raw(rk, hk, n_powers, in, tag_len, rounds, out_plain, out_tag_diff, mem == TAE_MEM_DEVICE,
                              key_bits);
    });
}

int tae_aesx_gcm_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                             const tae_bit *const *hk, size_t n_powers, const tae_gcm_frame *frames, size_t n_frames,
                             int tag_len, int rounds, tae_bit **out_plain, tae_bit **out_tag_diff) {
    return guarded([&] {
        require((expanded_key && hk && out_tag_diff) || !n_frames, "null");
        const size_t kw = key_cts(key_bits);
        const std::vector<tae::Context::GcmFrameIn> in = gcm_frames_in(frames, n_frames);
        require_xts_server(ctx);
        if (!n_frames) return;
        const tae::Context::GcmBits res =
            ctx->ctx->aes_gcm(unwrap(expanded_key, kw), unwrap(hk, n_powers * 128), in, tag_len, rounds, key_bits);
        require(out_plain || res.plain.empty(), "null");
        emit(res.plain, out_plain);
        emit(res.tag_diff, out_tag_diff);
    });
}

/* ---- GCM over key tables.  The frames are validated on the host before the context is looked at,
 * so their refusals need no device ---- */
extern "C++" {
namespace {
std::vector<tae::Context::GcmStreamIn> gcm_streams_in(const tae_gcm_stream *streams, size_t n_streams) {
    require(streams || !n_streams, "null");
    std::vector<tae::Context::GcmStreamIn> v(n_streams);
    for (size_t i = 0; i < n_streams; i++)
        v[i] = {streams[i].key,
                {streams[i].iv, streams[i].iv_len, streams[i].aad, streams[i].aad_len, streams[i].data, streams[i].len}};
    return v;
}
}  // namespace
}  // extern "C++"

int tae_aesm_ghash_key_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys, int n_powers,
                           int rounds, uint64_t *htable, int mem) {
    return guarded([&] {
        require((table && htable) || !n_keys, "null");
        key_cts(key_bits);
        require_xts_server(ctx);
        ctx->ctx->aes_ghash_key_multi_raw(table, n_keys, n_powers, rounds, htable, mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_ghash_key(const tae_context *ctx, int key_bits, const tae_bit *const *table, size_t n_keys, int n_powers,
                       int rounds, tae_bit **htable) {
    return guarded([&] {
        require((table && htable) || !n_keys, "null");
        const size_t kw = key_cts(key_bits);
        require_xts_server(ctx);
        if (!n_keys) return;
        emit(ctx->ctx->aes_ghash_key_multi(unwrap(table, n_keys * kw), n_keys, n_powers, rounds, key_bits), htable);
    });
}

int tae_aesm_gcm_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *table, size_t n_keys,
                                 const uint64_t *htable, size_t n_powers, const tae_gcm_stream *streams, size_t n_streams,
                                 int tag_len, int rounds, uint64_t *out_plain, uint64_t *out_tag_diff, int mem) {
    return guarded([&] {
        require((table && htable && out_tag_diff) || !n_streams, "null");
        key_cts(key_bits);
        const std::vector<tae::Context::GcmStreamIn> in = gcm_streams_in(streams, n_streams);
        std::vector<int32_t> slots;
        tae::gcm_multi_frames(in, n_keys, n_powers, tag_len, slots);
        require_xts_server(ctx);
        ctx->ctx->aes_gcm_multi_raw(table, n_keys, htable, n_powers, in, tag_len, rounds, out_plain, out_tag_diff,
                                    mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesm_gcm_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *table, size_t n_keys,
                             const tae_bit *const *htable, size_t n_powers, const tae_gcm_stream *streams,
                             size_t n_streams, int tag_len, int rounds, tae_bit **out_plain, tae_bit **out_tag_diff) {
    return guarded([&] {
        require((table && htable && out_tag_diff) || !n_streams, "null");
        key_cts(key_bits);
        const std::vector<tae::Context::GcmStreamIn> in = gcm_streams_in(streams, n_streams);
        std::vector<int32_t> slots;
        tae::gcm_multi_frames(in, n_keys, n_powers, tag_len, slots);
        require_xts_server(ctx);
        if (!n_streams) return;
        const tae::Context::GcmBits res = ctx->ctx->aes_gcm_multi(bit_at(table), n_keys, bit_at(htable), n_powers, in,
                                                                  tag_len, rounds, key_bits);
        require(out_plain || res.plain.empty(), "null");
        emit(res.plain, out_plain);
        emit(res.tag_diff, out_tag_diff);
    });
}

/* ---- frames beyond one table: segmented GHASH ---- */
int tae_aesx_gcm_long_rows(const uint8_t *iv, size_t iv_len, const uint8_t *aad, size_t aad_len, const uint8_t *data,
                           size_t data_len, int tag_len, size_t n_powers, size_t seg, size_t n_strides,
                           int32_t *row_sources, int32_t *row_chunks) {
    return guarded([&] {
        require(iv && row_sources && row_chunks && (aad || !aad_len) && (data || !data_len), "null");
        tae::GcmFrame f;
        throw_gcm_format(tae::gcm_format(iv, iv_len, aad, aad_len, data, data_len, tag_len, f));
        if (seg < 1) throw tae::ModelError{TAE_E_PARAM, "seg must be in 1..=n_powers"};
        const size_t C = tae::gcm_long_segments(f.m(), seg);
        std::vector<std::vector<int32_t>> rows;
        bool noise = false;
        for (size_t c = 0; c < C; c++) {
            if (c) tae::gcm_segment_rows(f, seg, c, 128, rows);
            else tae::gcm_long_final_rows(f, seg, 0, rows);
            noise = noise || !(c ? tae::gcm_inner_rows_ok(rows) : tae::gcm_final_rows_ok(rows));
            for (size_t r = 0; r < 128; r++) {
                const bool in = r < rows.size();
                row_sources[c * 128 + r] = in ? (int32_t)rows[r].size() : 0;
                row_chunks[c * 128 + r] =
                    !in ? 0 : (int32_t)(c ? tae::gcm_inner_chunks(rows[r].size()) : tae::gcm_row_chunks(rows[r].size()));
            }
        }
        switch (tae::gcm_long_shape_check(f.m(), seg, n_powers, n_strides)) {
            case tae::GCM_LONG_SEG: throw tae::ModelError{TAE_E_PARAM, "seg must be in 1..=n_powers"};
            case tae::GCM_LONG_STRIDES:
                throw tae::ModelError{TAE_E_PARAM, "n_strides must be in 1..=64 and at least the frame's segments less one"};
            default: break;
        }
        if (noise) throw tae::ModelError{TAE_E_NOISE, "a row needs more than 64 refreshed chunks"};
    });
}

int tae_aesx_gcm_long_noise_schedule_check(int param_set, int key_bits, int rounds, int n_powers, size_t seg,
                                           int n_strides, size_t aad_len, size_t data_len) {
    return guarded([&] {
        const tae::Params p = params_of(param_set);
        const size_t kw = key_cts(key_bits);
        const int nk = tae::aes_nk(key_bits), nr = tae::aes_nr(key_bits);
        if (p.model != 1) throw tae::ModelError{TAE_E_PARAM, "GCM runs on the 1-bit WoP-PBS parameter sets only"};
        std::vector<tae::NoiseLevel> key((size_t)nk * 32);
        for (auto &x : key) x = tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        const std::vector<tae::NoiseLevel> rk = tae::aes_key_expand_noise_schedule(key, nk, p.max_noise_sq);
        require(rk.size() == kw, "expanded key size");
        const tae::GhashKeyNoise hk = tae::aes_ghash_key_noise_schedule(rk, n_powers, rounds, p.max_noise_sq, nr);
        const tae::GhashKeyNoise sk = tae::aes_ghash_stride_key_noise_schedule(hk.table, seg, n_strides, p.max_noise_sq);
        // a frame of the given sizes with dense blocks: every byte 0xA5
        const uint8_t iv[12] = {};
        const std::vector<uint8_t> aad(aad_len, 0xA5), data(data_len, 0xA5);
        tae::GcmFrame f;
        throw_gcm_format(tae::gcm_format(iv, 12, aad.data(), aad_len, data.data(), data_len, 16, f));
        tae::aes_gcm_long_noise_schedule(rk, hk.table, sk.table, seg, f, rounds, p.max_noise_sq, nr);
    });
}

int tae_aesx_ghash_stride_key_raw(const tae_context *ctx, const uint64_t *hk, size_t n_powers, size_t seg, int n_strides,
                                  uint64_t *sk, int mem) {
    return guarded([&] {
        require(hk && sk, "null");
        require_xts_server(ctx);
        ctx->ctx->aes_ghash_stride_key_raw(hk, n_powers, seg, n_strides, sk, mem == TAE_MEM_DEVICE);
    });
}

int tae_aesx_ghash_stride_key(const tae_context *ctx, const tae_bit *const *hk, size_t n_powers, size_t seg, int n_strides,
                              tae_bit **sk) {
    return guarded([&] {
        require(hk && sk, "null");
        require_xts_server(ctx);
        emit(ctx->ctx->aes_ghash_stride_key(unwrap(hk, n_powers * 128), seg, n_strides), sk);
    });
}

int tae_aesx_gcm_long_transcipher_raw(const tae_context *ctx, int key_bits, const uint64_t *rk, const uint64_t *hk,
                                      size_t n_powers, const uint64_t *sk, size_t n_strides, size_t seg,
                                      const tae_gcm_frame *frames, size_t n_frames, int tag_len, int rounds,
                                      uint64_t *out_plain, uint64_t *out_tag_diff, int mem) {
    return guarded([&] {
        require((rk && hk && sk && out_tag_diff) || !n_frames, "null");
        key_cts(key_bits);
        const std::vector<tae::Context::GcmFrameIn> in = gcm_frames_in(frames, n_frames);
        require_xts_server(ctx);
        ctx->ctx->aes_gcm_long_raw(rk, hk, n_powers, sk, n_strides, seg, in, tag_len, rounds, out_plain, out_tag_diff,
                                   mem == TAE_MEM_DEVICE, key_bits);
    });
}

int tae_aesx_gcm_long_transcipher(const tae_context *ctx, int key_bits, const tae_bit *const *expanded_key,
                                  const tae_bit *const *hk, size_t n_powers, const tae_bit *const *sk, size_t n_strides,
                                  size_t seg, const tae_gcm_frame *frames, size_t n_frames, int tag_len, int rounds,
                                  tae_bit **out_plain, tae_bit **out_tag_diff) {
    return guarded([&] {
        require((expanded_key && hk && sk && out_tag_diff) || !n_frames, "null");
        const size_t kw = key_cts(key_bits);
        const std::vector<tae::Context::GcmFrameIn> in = gcm_frames_in(frames, n_frames);
        require_xts_server(ctx);
        if (!n_frames) return;
        const tae::Context::GcmBits res =
            ctx->ctx->aes_gcm_long(unwrap(expanded_key, kw), unwrap(hk, n_powers * 128), unwrap(sk, n_strides * 128), seg,
                                   in, tag_len, rounds, key_bits);
        require(out_plain || res.plain.empty(), "null");
        emit(res.plain, out_plain);
        emit(res.tag_diff, out_tag_diff);
    });
}

int tae_stage_gf128_square(const tae_context *ctx, const uint64_t *in, size_t count, uint64_t *out, int mem) {
    return guarded([&] {
        require((in && out) || !count, "null");
        require_xts_server(ctx);
        ctx->ctx->gf128_square_raw(in, count, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_stage_gf128_product(const tae_context *ctx, const uint64_t *a, const uint64_t *b, size_t count, uint64_t *out,
                            int mem) {
    return guarded([&] {
        require((a && b && out) || !count, "null");
        require_xts_server(ctx);
        ctx->ctx->gf128_product_raw(a, b, count, out, mem == TAE_MEM_DEVICE);
    });
}

/* ---- AEAD open: the verdict bit and the verdict-gated payload (no counterpart in the reference) ---- */
extern "C++" {
namespace {
void require_tag_len(int tag_len) {
    if (!tae::aead_tag_len_ok(tag_len)) throw tae::ModelError{TAE_E_PARAM, "a tag is 4 .. 16 bytes, and even or 13 or 15"};
}

size_t payload_bytes(const size_t *payload_lens, size_t n_frames) {
    size_t total = 0;
    for (size_t f = 0; f < n_frames; f++) total += payload_lens[f];
    return total;
}
}  // namespace
}  // extern "C++"

int tae_aead_open_plan(int tag_len, const size_t *payload_lens, size_t n_frames, int *levels, size_t *verdict_groups,
                       size_t *gate_groups) {
    return guarded([&] {
        require(levels && verdict_groups && gate_groups && (payload_lens || !n_frames), "null");
        require_tag_len(tag_len);
        const tae::VerdictPlan v = tae::aead_verdict_plan(tag_len, 1);
        *levels = v.levels();
        for (int l = 0; l < v.levels(); l++) verdict_groups[l] = v.groups[l];
        *gate_groups = payload_bytes(payload_lens, n_frames);
    });
}

int tae_aead_open_noise_schedule_check(int param_set, int tag_len, uint64_t plain_level, uint64_t diff_level) {
    return guarded([&] {
        const tae::Params p = params_of(param_set);
        if (p.model != 1)
            throw tae::ModelError{TAE_E_PARAM, "the AEAD open runs on the 1-bit WoP-PBS parameter sets only"};
        require_tag_len(tag_len);
        // one frame of one payload byte
        const size_t one = 1;
        const tae::VerdictPlan v = tae::aead_verdict_plan(tag_len, 1);
        const tae::GatePlan g = tae::aead_gate_plan(&one, 1);
        std::vector<tae::NoiseLevel> plain(8), diff(v.bits[0]);
        for (auto &x : plain) x = tae::NoiseLevel::with_noise_level(plain_level, tae::next_ct_id());
        for (auto &x : diff) x = tae::NoiseLevel::with_noise_level(diff_level, tae::next_ct_id());
        tae::aead_open_noise_schedule(plain, diff, v, g, p.max_noise_sq);
    });
}

int tae_aead_verdict_raw(const tae_context *ctx, const uint64_t *tag_diff, size_t n_frames, int tag_len, uint64_t *ok,
                         int mem) {
    return guarded([&] {
        require((tag_diff && ok) || !n_frames, "null");
        require_tag_len(tag_len);
        require_xts_server(ctx);
        ctx->ctx->aead_verdict_raw(tag_diff, n_frames, tag_len, ok, mem == TAE_MEM_DEVICE);
    });
}

int tae_aead_open_raw(const tae_context *ctx, const uint64_t *plain, const size_t *payload_lens, const uint64_t *tag_diff,
                      size_t n_frames, int tag_len, uint64_t *out_plain, uint64_t *out_ok, int mem) {
    return guarded([&] {
        require((payload_lens && tag_diff && out_ok) || !n_frames, "null");
        require((plain && out_plain) || !payload_bytes(payload_lens, n_frames), "null");
        require_tag_len(tag_len);
        require_xts_server(ctx);
        ctx->ctx->aead_open_raw(plain, payload_lens, tag_diff, n_frames, tag_len, out_plain, out_ok, mem == TAE_MEM_DEVICE);
    });
}

int tae_aead_open(const tae_context *ctx, const tae_bit *const *plain, const size_t *payload_lens,
                  const tae_bit *const *tag_diff, size_t n_frames, int tag_len, tae_bit **out_plain, tae_bit **out_ok) {
    return guarded([&] {
        require((payload_lens && tag_diff && out_ok) || !n_frames, "null");
        const size_t n_bytes = payload_bytes(payload_lens, n_frames);
        require((plain && out_plain) || !n_bytes, "null");
        require_tag_len(tag_len);
        require_xts_server(ctx);
        if (!n_frames) return;
        const tae::Context::OpenBits res = ctx->ctx->aead_open(
            unwrap(plain, n_bytes * 8), payload_lens, unwrap(tag_diff, n_frames * 8 * (size_t)tag_len), n_frames, tag_len);
        emit(res.plain, out_plain);
        emit(res.ok, out_ok);
    });
}

int tae_aes_sbox_pbs_encrypt_blocks(const tae_context *ctx, const tae_bit *const *expanded_key,
                                    const tae_bit *const *blocks, size_t n_blocks, int rounds, tae_bit **out) {
    return guarded([&] {
        require(ctx && expanded_key && blocks && out, "null");
        emit(ctx->ctx->aes_encrypt_blocks(unwrap(expanded_key, 44 * 32), unwrap(blocks, 128 * n_blocks), n_blocks,
                                          rounds, tae::AesDriver::SboxPbs),
             out);
    });
}

int tae_aes_sbox_pbs_key_schedule(const tae_context *ctx, const tae_bit *const *key, tae_bit **expanded) {
    return guarded([&] {
        require(ctx && key && expanded, "null");
        emit(ctx->ctx->aes_key_schedule(unwrap(key, 128), tae::AesDriver::SboxPbs), expanded);
    });
}

int tae_aes_sbox_pbs_encrypt_blocks_raw(const tae_context *ctx, const uint64_t *rk, const uint64_t *blocks,
                                        size_t n_blocks, int rounds, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && rk && blocks && out, "null");
        ctx->ctx->aes_encrypt_blocks_raw(rk, blocks, n_blocks, rounds, out, mem == TAE_MEM_DEVICE,
                                         tae::AesDriver::SboxPbs);
    });
}

int tae_aes_sbox_pbs_key_schedule_raw(const tae_context *ctx, const uint64_t *key, uint64_t *expanded, int mem) {
    return guarded([&] {
        require(ctx && key && expanded, "null");
        ctx->ctx->aes_key_schedule_raw(key, expanded, mem == TAE_MEM_DEVICE, tae::AesDriver::SboxPbs);
    });
}

int tae_aes_noise_schedule_check(int param_set, int driver, int rounds) {
    return guarded([&] {
        const tae::Params p = params_of(param_set);
        require(driver == TAE_DRIVER_GAL_MUL || driver == TAE_DRIVER_SBOX_PBS, "unknown driver");
        if (rounds < 1 || rounds > 10) throw tae::ModelError{TAE_E_PARAM, "rounds must be in 1..=10"};
        if (p.model == 2) return;  // shortint_1bit: unchecked adds, no bookkeeping to fail
        std::vector<tae::NoiseLevel> rk(44 * 32), blk(128);
        for (auto &x : rk) x = p.model == 8 ? tae::NoiseLevel{1, {}} : tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        for (auto &x : blk) x = p.model == 8 ? tae::NoiseLevel{1, {}} : tae::NoiseLevel::with_noise_level(1, tae::next_ct_id());
        if (p.model == 8)
            tae::aes8_noise_schedule(rk, blk, rounds, p.max_noise_sq);
        else if (driver == TAE_DRIVER_SBOX_PBS)
            tae::sbox_pbs_noise_schedule(rk, blk, rounds, p.max_noise_sq);
        else
            tae::aes_noise_schedule(rk, blk, rounds, p.max_noise_sq);
    });
}


/* ---- shortint_1bit model ---- */
int tae_s1_test_vector_from_fn(int param_set, uint64_t f0, uint64_t f1, uint64_t *tv) {
    return guarded([&] {
        require(tv, "null");
        const tae::Params p = params_of(param_set);
        require(p.model == 2, "test vectors belong to the shortint_1bit parameter set");
        require(f0 <= 1 && f1 <= 1, "function values must be 0 or 1");
        tae::s1_test_vector(p, f0, f1, tv);
    });
}

int tae_s1_bootstrap(const tae_context *ctx, const uint64_t *in, size_t count, const uint64_t *tvs, size_t n_tv,
                     uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && (in || !count) && tvs && (out || !count), "null");
        if (count) ctx->ctx->s1_bootstrap_raw(in, count, tvs, n_tv, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_s1_packing_keyswitch(const tae_context *ctx, const uint64_t *cts, size_t count, uint64_t *glwe, int mem) {
    return guarded([&] {
        require(ctx && cts && glwe, "null");
        ctx->ctx->s1_packing_keyswitch_raw(cts, count, glwe, mem == TAE_MEM_DEVICE);
    });
}

int tae_s1_test_vectors_from_ciphertexts(const tae_context *ctx, const uint64_t *ct0, const uint64_t *ct1, size_t count,
                                         uint64_t *tvs, int mem) {
    return guarded([&] {
        require(ctx && (count == 0 || (ct0 && ct1 && tvs)), "null");
        if (count) ctx->ctx->s1_test_vectors_from_ciphertexts_raw(ct0, ct1, count, tvs, mem == TAE_MEM_DEVICE);
    });
}

int tae_s1_multivariate(const tae_context *ctx, const uint64_t *bits, size_t groups, int nbits,
                        const uint64_t *f_tables, int n_fn, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && f_tables && (groups == 0 || (bits && out)), "null");
        if (groups) ctx->ctx->s1_multivariate_raw(bits, groups, nbits, f_tables, n_fn, out, mem == TAE_MEM_DEVICE);
    });
}

/* ---- packed ciphertext I/O (glwe_pack.hpp) ---- */
static tae::Params pack_params(int param_set) {
    const tae::Params p = params_of(param_set);
    if (p.id != tae::SQRD_LVL_64)
        throw tae::ModelError{TAE_E_PARAM, "packed ciphertext I/O is built for params_sqrd_lvl_64 only"};
    return p;
}

// A server call: the arguments first, then the device (a machine without one has no context to pass).
static void require_pack_server(const tae_context *ctx, const void *in, size_t count, const void *out) {
    require(in && out, "null");
    require(count > 0, "a packed call needs at least one bit");
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0)
        throw tae::ModelError{TAE_E_NODEV, "no GPU available: the HIP path has no CPU fallback"};
    require(ctx != nullptr, "null");
}

int tae_packed_len(int param_set, size_t count, size_t *glwes, size_t *words) {
    return guarded([&] {
        const tae::Params p = pack_params(param_set);
        require(count > 0, "a packed call needs at least one bit");
        const size_t G = tae::glwe_pack::glwe_count(count, p.N);
        if (glwes) *glwes = G;
        if (words) *words = G * p.glwe_len();
    });
}

int tae_encrypt_packed_raw(const tae_client_key *ck, const uint8_t *bits, size_t count, uint64_t start_index,
                           uint64_t *glwes) {
    return guarded([&] {
        require(ck && bits && glwes, "null");
        const tae::Params p = pack_params(ck->ck.p.id);
        require(count > 0, "a packed call needs at least one bit");
        for (size_t i = 0; i < count; i++) require(bits[i] < 2, "cleartext out of bounds");
        const size_t G = tae::glwe_pack::glwe_count(count, p.N);
        const uint64_t first = raw_index_range(ck, G, start_index);
        for (size_t g = 0; g < G; g++)
            ck->ck.encrypt_packed_at(bits + g * p.N, std::min<size_t>(p.N, count - g * p.N), first + g,
                                     glwes + g * p.glwe_len());
    });
}

int tae_decrypt_packed_raw(const tae_client_key *ck, const uint64_t *glwes, size_t count, uint8_t *bits) {
    return guarded([&] {
        require(ck && glwes && bits, "null");
        const tae::Params p = pack_params(ck->ck.p.id);
        require(count > 0, "a packed call needs at least one bit");
        const size_t G = tae::glwe_pack::glwe_count(count, p.N);
        for (size_t g = 0; g < G; g++)
            ck->ck.decrypt_packed(glwes + g * p.glwe_len(), std::min<size_t>(p.N, count - g * p.N), bits + g * p.N);
    });
}

int tae_packed_narrow(const uint64_t *wide, size_t words, uint32_t *narrow) {
    return guarded([&] {
        require(wide && narrow, "null");
        for (size_t i = 0; i < words; i++) narrow[i] = tae::glwe_pack::narrow_word(wide[i]);
    });
}

int tae_packed_widen(const uint32_t *narrow, size_t words, uint64_t *wide) {
    return guarded([&] {
        require(narrow && wide, "null");
        for (size_t i = 0; i < words; i++) wide[i] = tae::glwe_pack::widen_word(narrow[i]);
    });
}

int tae_unpack_bits_raw(const tae_context *ctx, const uint64_t *glwes, size_t count, uint64_t *bits, int mem) {
    return guarded([&] {
        require_pack_server(ctx, glwes, count, bits);
        ctx->ctx->unpack_bits_raw(glwes, count, bits, mem == TAE_MEM_DEVICE);
    });
}

int tae_pack_bits_raw(const tae_context *ctx, const uint64_t *bits, size_t count, uint64_t *glwes, int mem) {
    return guarded([&] {
        require_pack_server(ctx, bits, count, glwes);
        ctx->ctx->pack_bits_raw(bits, count, glwes, mem == TAE_MEM_DEVICE);
    });
}

int tae_unpack_bits(const tae_context *ctx, const uint64_t *glwes, size_t count, tae_bit **out) {
    return guarded([&] {
        require_pack_server(ctx, glwes, count, out);
        emit(ctx->ctx->unpack_bits(glwes, count), out);
    });
}

int tae_pack_bits(const tae_context *ctx, const tae_bit *const *bits, size_t count, uint64_t *glwes) {
    return guarded([&] {
        require_pack_server(ctx, bits, count, glwes);
        ctx->ctx->require_pack(count);
        ctx->ctx->pack_bits(unwrap(bits, count), glwes);
    });
}

int tae_last_pack_time(const tae_context *ctx, double *ms) {
    return guarded([&] {
        require(ctx && ms, "null");
        *ms = ctx->ctx->engine().last_times().pack;
    });
}

int tae_stage_pack_pfks(const tae_context *ctx, const uint64_t *bits, size_t count, uint64_t *out, int mem) {
    return guarded([&] {
        require_pack_server(ctx, bits, count, out);
        ctx->ctx->pack_pfks_raw(bits, count, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_stage_keyswitch(const tae_context *ctx, const uint64_t *in, size_t count, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && in && out, "null");
        ctx->ctx->keyswitch_raw(in, count, out, mem == TAE_MEM_DEVICE);
    });
}

int tae_stage_pbs_shift_boolean(const tae_context *ctx, const uint64_t *small, size_t count, int level, uint64_t *big,
                                int mem) {
    return guarded([&] {
        require(ctx && small && big, "null");
        require(level >= 1 && level <= ctx->ctx->params().cbs_l, "level out of range");
        ctx->ctx->pbs_shift_boolean_raw(small, count, level, big, mem == TAE_MEM_DEVICE);
    });
}

int tae_stage_bootstrap(const tae_context *ctx, const uint64_t *small, size_t count, const uint64_t *lut_glwe,
                        uint64_t *big, int mem) {
    return guarded([&] {
        require(ctx && small && lut_glwe && big, "null");
        ctx->ctx->bootstrap_raw(small, count, lut_glwe, big, mem == TAE_MEM_DEVICE);
    });
}

int tae_stage_pfks_ggsw(const tae_context *ctx, const uint64_t *big, size_t count, int level, uint64_t *ggsw, int mem) {
    return guarded([&] {
        require(ctx && big && ggsw, "null");
        require(level >= 1 && level <= ctx->ctx->params().cbs_l, "level out of range");
        ctx->ctx->pfks_ggsw_raw(big, count, level, ggsw, mem == TAE_MEM_DEVICE);
    });
}

int tae_stage_ggsw_fourier(const tae_context *ctx, const uint64_t *ggsw, size_t count, double *ggsw_f, int mem) {
    return guarded([&] {
        require(ctx && ggsw && ggsw_f, "null");
        ctx->ctx->ggsw_fourier_raw(ggsw, count, reinterpret_cast<tae::cplx *>(ggsw_f), mem == TAE_MEM_DEVICE);
    });
}

int tae_stage_vertical_packing(const tae_context *ctx, const double *ggsw_f, size_t groups, int n_in,
                               const uint64_t *lut, int n_out, uint64_t *out, int mem) {
    return guarded([&] {
        require(ctx && ggsw_f && lut && out, "null");
        require(n_in >= 1 && n_out >= 1, "n_in and n_out must be at least 1");
        ctx->ctx->vertical_packing_raw(reinterpret_cast<const tae::cplx *>(ggsw_f), groups, n_in, lut, n_out, out,
                                       mem == TAE_MEM_DEVICE);
    });
}

int tae_synchronize(const tae_context *ctx) {
    return guarded([&] {
        require(ctx, "null");
        ctx->ctx->engine().synchronize();
    });
}

int tae_set_caller_stream(tae_context *ctx, void *stream) {
    return guarded([&] {
        require(ctx, "null");
        std::lock_guard<std::mutex> g(ctx->ctx->mutex());  // the context's entry points hold the same lock
        ctx->ctx->engine().set_caller_stream((hipStream_t)stream);
    });
}

int tae_set_timing(const tae_context *ctx, int on) {
    return guarded([&] {
        require(ctx, "null");
        require(on >= 0 && on <= 2, "timing mode is 0, 1 or 2");
        ctx->ctx->engine().set_timing(on);
    });
}

int tae_last_stage_times_v4(const tae_context *ctx, double *v12) {
    return guarded([&] {
        require(ctx && v12, "null");
        const auto &t = ctx->ctx->engine().last_times();
        const double v[12] = {t.keyswitch, t.pbs,    t.pfks,         t.ggsw_fft, t.vertical_packing,
                              t.extract,   t.linear, (double)t.pbs_launches, t.pbs_main, t.pbs_main_cts,
                              t.pbs_clock_launches ? t.pbs_clock_ghz_sum / t.pbs_clock_launches : 0.0,
                              (double)t.pbs_clock_launches};
        for (int i = 0; i < 12; i++) v12[i] = v[i];
    });
}

int tae_last_pfks_kernel(const tae_context *ctx, char *name, size_t cap) {
    return guarded([&] {
        require(ctx && name && cap, "null");
        const char *k = ctx->ctx->engine().last_pfks_kernel();
        require(strlen(k) < cap, "name buffer too small");
        strcpy(name, k);
    });
}

int tae_last_stage_times_v2(const tae_context *ctx, float *ms8) {
    return guarded([&] {
        require(ctx && ms8, "null");
        const auto &t = ctx->ctx->engine().last_times();
        const float v[8] = {t.keyswitch, t.pbs, t.pfks, t.ggsw_fft, t.vertical_packing, t.extract, t.linear,
                            (float)t.pbs_launches};
        for (int i = 0; i < 8; i++) ms8[i] = v[i];
    });
}

int tae_last_stage_times_v3(const tae_context *ctx, double *v10) {
    return guarded([&] {
        require(ctx && v10, "null");
        const auto &t = ctx->ctx->engine().last_times();
        const double v[10] = {t.keyswitch, t.pbs,    t.pfks,         t.ggsw_fft, t.vertical_packing,
                              t.extract,   t.linear, (double)t.pbs_launches, t.pbs_main, t.pbs_main_cts};
        for (int i = 0; i < 10; i++) v10[i] = v[i];
    });
}

int tae_last_stage_times(const tae_context *ctx, float *ms5) {
    return guarded([&] {
        require(ctx && ms5, "null");
        const auto &t = ctx->ctx->engine().last_times();
        ms5[0] = t.keyswitch;
        ms5[1] = t.pbs;
        ms5[2] = t.pfks;
        ms5[3] = t.ggsw_fft;
        ms5[4] = t.vertical_packing;
    });
}

}  // extern "C"
