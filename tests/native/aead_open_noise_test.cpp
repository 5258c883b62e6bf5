// The host model's bookkeeping of the AEAD open (model.cpp aead_open_noise_schedule) called in the product library, no
// GPU call: verdict bits at 8 and gated payload bits at 9, fresh ids that are distinct from each other
// and from the inputs', and TAE_E_NOISE for an input one above the cap.  Built and run by tests/test_aead_open.py.
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../tfhe-aes-2_amd/csrc/aead_open.hpp"

namespace tae {
// model.hpp's declarations (the header itself needs the HIP runtime's)
struct ModelError {
    int code;
    std::string msg;
};
struct NoiseLevel {
    uint64_t noise_level_squared = 0;
    std::vector<uint64_t> components;
    void add_assign(const NoiseLevel &rhs, uint64_t max_noise_sq);
};
uint64_t next_ct_id();
struct AeadOpenNoise {
    std::vector<NoiseLevel> plain, ok;
};
AeadOpenNoise aead_open_noise_schedule(const std::vector<NoiseLevel> &plain, const std::vector<NoiseLevel> &diff,
                                       const VerdictPlan &verdict, const GatePlan &gate, uint64_t max_noise_sq);
}  // namespace tae

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                \
        }                                                           \
    } while (0)

static std::vector<tae::NoiseLevel> at_level(size_t n, uint64_t level) {
    std::vector<tae::NoiseLevel> v(n);
    for (auto &x : v) x = {level, {tae::next_ct_id()}};
    return v;
}

template <class F>
static int code_of(F fn) {
    try {
        fn();
    } catch (const tae::ModelError &e) {
        return e.code;
    }
    return 0;
}

int main() {
    const uint64_t max = 64;  // params_sqrd_lvl_64
    const int E_NOISE = 1, E_ARG = 5;
    for (int tag_len : {4, 13, 16}) {
        const size_t lens[] = {17, 0, 3}, n = 3;
        const tae::VerdictPlan vp = tae::aead_verdict_plan(tag_len, n);
        const tae::GatePlan gp = tae::aead_gate_plan(lens, n);
        // a CTR payload bit is at 8 + 1, a GCM difference bit at its chunk count: up to the cap
        const std::vector<tae::NoiseLevel> plain = at_level(gp.n_bytes() * 8, 9), diff = at_level(n * vp.bits[0], max);
        const tae::AeadOpenNoise out = tae::aead_open_noise_schedule(plain, diff, vp, gp, max);
        CHECK(out.ok.size() == n && out.plain.size() == plain.size());
        std::set<uint64_t> ids, in_ids;
        for (const auto &x : plain) in_ids.insert(x.components[0]);
        for (const auto &x : diff) in_ids.insert(x.components[0]);
        for (const auto &x : out.ok) {
            CHECK(x.noise_level_squared == 8 && x.components.size() == 1);
            ids.insert(x.components[0]);
        }
        for (const auto &x : out.plain) {
            CHECK(x.noise_level_squared == 9 && x.components.size() == 1);
            ids.insert(x.components[0]);
        }
        CHECK(ids.size() == out.ok.size() + out.plain.size());
        for (uint64_t id : ids) CHECK(!in_ids.count(id));
        // the outputs hold no input's id, so a gated bit may be added to its own input and to a verdict
        tae::NoiseLevel v = out.plain[0];
        v.add_assign(plain[0], max);
        v.add_assign(out.ok[0], max);
        CHECK(v.noise_level_squared == 9 + 9 + 8);
        // the verdict alone: no payload
        tae::GatePlan none;
        none.n_frames = n;
        const tae::AeadOpenNoise vo = tae::aead_open_noise_schedule({}, diff, vp, none, max);
        CHECK(vo.ok.size() == n && vo.plain.empty() && vo.ok[1].noise_level_squared == 8);
        // one input one above the cap: a difference bit (the last one), a payload bit (the last one)
        std::vector<tae::NoiseLevel> bad = diff;
        bad.back().noise_level_squared = max + 1;
        CHECK(code_of([&] { tae::aead_open_noise_schedule(plain, bad, vp, gp, max); }) == E_NOISE);
        bad = plain;
        bad.back().noise_level_squared = max + 1;
        CHECK(code_of([&] { tae::aead_open_noise_schedule(bad, diff, vp, gp, max); }) == E_NOISE);
        CHECK(code_of([&] { tae::aead_open_noise_schedule(at_level(plain.size(), max), diff, vp, gp, max); }) == 0);
        // a cap below 8: the level-1 inputs and the gate's verdict input are refused; at 8 they pass
        CHECK(code_of([&] { tae::aead_open_noise_schedule(at_level(plain.size(), 1), at_level(diff.size(), 1), vp, gp, 7); }) ==
              E_NOISE);
        CHECK(code_of([&] { tae::aead_open_noise_schedule(at_level(plain.size(), 1), at_level(diff.size(), 1), vp, gp, 8); }) == 0);
        // bits that do not match the plans
        CHECK(code_of([&] { tae::aead_open_noise_schedule(plain, at_level(diff.size() - 1, 1), vp, gp, max); }) == E_ARG);
        CHECK(code_of([&] { tae::aead_open_noise_schedule(at_level(8, 1), diff, vp, gp, max); }) == E_ARG);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
