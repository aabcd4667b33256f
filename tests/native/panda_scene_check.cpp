// Stand-alone check (its own main) of the host side of m3_set_panda_scene (csrc/panda_scene.hpp, csrc/panda_dyn.hpp):
// make_panda_scene with masses, make_panda_scene_rt and the per-field validation.  Built twice by
// tests/test_panda_scene_cpu.py -- plain and with -fsanitize=address,undefined -- and run directly.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -Itests/native/shim panda_scene_check.cpp -o panda_scene_check
#include "../../m3p2i_aip_amd/csrc/panda_scene.hpp"

#include <cstdio>
#include <cstring>
#include <limits>

static int fails = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } \
    } while (0)

static bool same_bits(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

int main() {
    using namespace m3;
    const float dt = 0.01f;
    const int substeps = 2;
    // 1. the masses as arguments: the defaults are what the literals gave
    PandaScene plain, masses;
    std::memset(&plain, 0, sizeof(plain));
    std::memset(&masses, 0, sizeof(masses));
    make_panda_scene(plain, dt, substeps);
    make_panda_scene(masses, dt, substeps, 6, PANDA_SCENE_DEFAULT.cube_m, PANDA_SCENE_DEFAULT.obs_m);
    CHECK(same_bits(&plain, &masses, sizeof(plain)));
    CHECK(plain.invm_cube == 1.0f / 0.125f && plain.invm_obs == 1.0f / 0.8f);
    {   // the oracle's order (panda_chain.c, m3o_panda_step): 1 / ((m * ((2 half) * (2 half))) / 6)
        volatile float m = 0.4f, half = 0.025f, om = 0.2f;
        const float side = 2.0f * half;
        const float want_I = 1.0f / ((m * (side * side)) / 6.0f);
        PandaScene s;
        make_panda_scene(s, dt, substeps, 6, 0.4f, 0.2f);
        CHECK(s.invm_cube == 1.0f / m && s.invI_cube == want_I && s.invm_obs == 1.0f / om);
        CHECK(same_bits(s.a, plain.a, sizeof(s.a)) && same_bits(s.pmax, plain.pmax, sizeof(s.pmax)) && s.h == plain.h);
    }
    // 2. make_panda_scene_rt: PandaScene's run-time part + the workspace, field for field
    {
        const PandaSceneRT d = make_panda_scene_rt(PANDA_SCENE_DEFAULT, dt, substeps);
        CHECK(same_bits(static_cast<const PandaScene*>(&d), &plain, sizeof(PandaScene)));
        CHECK(same_bits(d.base, PandaScene::base, sizeof(d.base)) && same_bits(d.table, PandaScene::table, sizeof(d.table)));
        CHECK(same_bits(d.shelf, PandaScene::shelf, sizeof(d.shelf)) && same_bits(d.obs_half, PandaScene::obs_half, sizeof(d.obs_half)));
        CHECK(d.mu == PandaScene::mu);
        m3_panda_scene p = PANDA_SCENE_DEFAULT;
        p.base[0] = -0.40f; p.table[2] = 0.99f; p.shelf[5] = 0.12f; p.obs_half[2] = 0.02f; p.mu = 0.3f; p.cube_m = 0.4f; p.obs_m = 0.2f;
        const PandaSceneRT r = make_panda_scene_rt(p, dt, substeps);
        CHECK(same_bits(r.base, p.base, sizeof(p.base)) && same_bits(r.table, p.table, sizeof(p.table)));
        CHECK(same_bits(r.shelf, p.shelf, sizeof(p.shelf)) && same_bits(r.obs_half, p.obs_half, sizeof(p.obs_half)) && r.mu == p.mu);
        PandaScene m;
        make_panda_scene(m, dt, substeps, 6, p.cube_m, p.obs_m);
        CHECK(same_bits(static_cast<const PandaScene*>(&r), &m, sizeof(PandaScene)));
        CHECK(!panda_scene_is_default(p) && !panda_scene_geometry_is_default(p));
        m3_panda_scene q = PANDA_SCENE_DEFAULT;
        q.cube_m = 0.4f;
        CHECK(!panda_scene_is_default(q) && panda_scene_geometry_is_default(q));
        CHECK(panda_scene_is_default(PANDA_SCENE_DEFAULT));
        q = PANDA_SCENE_DEFAULT;
        q.base[1] = -0.0f;      // (-0.0f is not the default 0.0f: the kernels would add it)
        CHECK(!panda_scene_geometry_is_default(q));
    }
    // 3. validation: every field, by its rule, named in the message
    {
        CHECK(panda_scene_fault(PANDA_SCENE_DEFAULT).empty());
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        static const char* const names[PANDA_SCENE_FLOATS] = {
            "base[0]", "base[1]", "base[2]", "table[0]", "table[1]", "table[2]", "table[3]", "table[4]", "table[5]",
            "shelf[0]", "shelf[1]", "shelf[2]", "shelf[3]", "shelf[4]", "shelf[5]", "obs_half[0]", "obs_half[1]", "obs_half[2]",
            "obs_m", "cube_m", "mu"};
        for (int i = 0; i < PANDA_SCENE_FLOATS; ++i) {
            CHECK(panda_scene_field_name(i) == names[i]);
            const bool position = i < 3 || (i < 15 && (i - 3) % 6 < 3);
            const bool friction = i == 20;
            for (float bad : {nan, inf, -inf}) {
                m3_panda_scene p = PANDA_SCENE_DEFAULT;
                float f[PANDA_SCENE_FLOATS];
                std::memcpy(f, &p, sizeof(f));
                f[i] = bad;
                std::memcpy(&p, f, sizeof(f));
                CHECK(panda_scene_fault(p) == std::string(names[i]) + " is not finite");
            }
            for (float v : {0.0f, -1.0f}) {
                m3_panda_scene p = PANDA_SCENE_DEFAULT;
                float f[PANDA_SCENE_FLOATS];
                std::memcpy(f, &p, sizeof(f));
                f[i] = v;
                std::memcpy(&p, f, sizeof(f));
                const std::string fault = panda_scene_fault(p);
                if (position || (friction && v == 0.0f)) CHECK(fault.empty());
                else if (friction) CHECK(fault == "mu must be >= 0");
                else CHECK(fault == std::string(names[i]) + " must be > 0");
            }
        }
    }
    if (fails == 0) std::printf("panda_scene_check: ok\n");
    return fails == 0 ? 0 : 1;
}
