// Host build of the panda_env task costs of the product's csrc/panda_dyn.hpp for the CPU tests
// (tests/test_panda_cost_weights_cpu.py): the device code of panda_cost, literal form and weighted form, row by row --
// without a GPU.
//   g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -Itests/native/shim panda_cost_host.cpp -o libpanda_cost_host.so
#include "../../m3p2i_aip_amd/csrc/panda_dyn.hpp"

// n rows of 30 floats as oracle.panda.make_obs lays them out: left3 left_q4 right3 | cube3 cube_q4 | cube0 3 cube_q_half0 4 |
// f_table2 f_shelf2 f_cubeB2.  wt: the seven floats of m3_panda_cost_weights -- the weighted overload of panda_cost -- or
// null: the literal form.  task 4 reach, 5 pick, 6 place; goal: 7 floats; cost [n], sample index k0 + i.
extern "C" void pcw_cost(const float* wt, int task, int multi_modal, int half_K, const float* goal, float pre_height_diff,
                         float tilt_cos_theta, const float* obs, int n, int k0, float* cost) {
    m3::PandaCostParams cp{};
    cp.task = task; cp.multi_modal = multi_modal; cp.half_K = half_K;
    for (int j = 0; j < 7; ++j) cp.goal[j] = goal[j];
    cp.pre_height_diff = pre_height_diff; cp.tilt_cos_theta = tilt_cos_theta;
    m3::PandaCostWeights w = m3::PANDA_COST_WEIGHTS_DEFAULT;
    if (wt) {
        w.reach_dist = wt[0]; w.reach_tilt = wt[1]; w.pick_goal = wt[2]; w.pick_ori = wt[3]; w.collision = wt[4];
        w.shelf_force = wt[5]; w.place_grip = wt[6];
    }
    for (int i = 0; i < n; ++i) {
        const float* r = obs + 30 * (long long)i;
        m3::PandaWorld p{};
        m3::PandaObs o{};
        for (int j = 0; j < 3; ++j) { o.left[j] = r[j]; o.right[j] = r[7 + j]; p.A.p[j] = r[10 + j]; }
        for (int j = 0; j < 4; ++j) { o.left_q[j] = r[3 + j]; p.A.q[j] = r[13 + j]; }
        for (int j = 0; j < 2; ++j) { p.f_table[j] = r[24 + j]; p.f_shelf[j] = r[26 + j]; p.f_cubeB[j] = r[28 + j]; }
        cost[i] = wt ? m3::panda_cost(cp, w, p, o, k0 + i, r + 17, r + 20) : m3::panda_cost(cp, p, o, k0 + i, r + 17, r + 20);
    }
}

extern "C" void pcw_default_weights(float* wt) {
    const m3::PandaCostWeights d = m3::PANDA_COST_WEIGHTS_DEFAULT;
    wt[0] = d.reach_dist; wt[1] = d.reach_tilt; wt[2] = d.pick_goal; wt[3] = d.pick_ori; wt[4] = d.collision;
    wt[5] = d.shelf_force; wt[6] = d.place_grip;
}
