// Host build of the product's csrc/point_cost.hpp for the CPU tests (tests/test_cost_weights_cpu.py): the device code of the
// point_env task costs, literal form and weighted form, world by world -- without a GPU.
//   g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -Itests/native/shim point_cost_host.cpp -o libpoint_cost_host.so
#include "../../m3p2i_aip_amd/csrc/point_cost.hpp"

// n worlds, rows of 8 floats: robot x y vx vy | box x y | dyn-obs contact force x y.  weighted != 0: point_cost_w with the nine
// floats of wt, else point_cost.  cost [n]; pend [n][4]: the pending suction force the evaluation leaves (robot x y, box x y;
// preset to a sentinel, so that a task that stages none shows).
extern "C" void pch_cost(int weighted, const float* wt, int task, int multi_modal, int half_K, float gx, float gy, float kp,
                         float thresh, int avoid, const float* worlds, int n, int k0, float* cost, float* pend) {
    m3::CostParams cp{};
    cp.task = task; cp.multi_modal = multi_modal; cp.half_K = half_K;
    cp.goal[0] = gx; cp.goal[1] = gy;
    cp.kp_suction = kp; cp.suction_thresh = thresh; cp.avoid_dyn_obs = avoid;
    m3::PointCostWeights w = m3::POINT_COST_WEIGHTS_DEFAULT;
    if (wt) {
        w.nav_dist = wt[0]; w.collision = wt[1]; w.robot_box = wt[2]; w.box_goal = wt[3]; w.push_dist = wt[4];
        w.push_align = wt[5]; w.pull_dist = wt[6]; w.pull_vel = wt[7]; w.pull_align = wt[8];
    }
    for (int i = 0; i < n; ++i) {
        const float* r = worlds + 8 * (long long)i;
        m3::PointWorld p{};
        p.rx = r[0]; p.ry = r[1]; p.rvx = r[2]; p.rvy = r[3];
        p.B.x = r[4]; p.B.y = r[5]; p.B.c = 1.0f;
        p.D.c = 1.0f;
        p.fcDx = r[6]; p.fcDy = r[7];
        float* f = pend + 4 * (long long)i;
        p.fRx = f[0]; p.fRy = f[1]; p.fBx = f[2]; p.fBy = f[3];
        cost[i] = weighted ? m3::point_cost_w(cp, w, p, k0 + i) : m3::point_cost(cp, p, k0 + i);
        f[0] = p.fRx; f[1] = p.fRy; f[2] = p.fBx; f[3] = p.fBy;
    }
}
