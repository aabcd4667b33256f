// prior_controllers.hpp -- the ancillary controllers of PRIOR SAMPLES (m3_set_prior_controller), host and device: the
// controllers of m3p2i_aip_amd/priors.py (go_to, push_behind) restated in IEEE binary32 with a FIXED operation order.  This text
// is the spec: the kernels (prior_controllers.hip) and a host build (tests/native/prior_controllers_host.cpp) compile it, and
// with contraction off (-ffp-contract=off, as for the rest of the library) and correctly rounded division and square root on
// both sides they agree bit for bit.  Includes nothing of the library: plain C++.
//
// The control is the robot's velocity command (vx, vy); the controllers roll the robot forward KINEMATICALLY (pos += u * dt).
// Left out on purpose: the clamp to the control limits (the rollout's select clamps: rollout_point_kernel.hpp) and contacts
// (what the rollout is for).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M3_PC_HD __host__ __device__ inline
#else
#define M3_PC_HD inline
#endif

namespace m3 {

// the values of m3_prior_controller::kind (include/m3p2i_hip_ext.h)
constexpr int PRIOR_CONTROLLER_GO_TO = 1, PRIOR_CONTROLLER_PUSH_BEHIND = 2;

// speed limit of sequence j: factor_j * min(|u_max[0]|, |u_max[1]|), so that the velocity vector stays inside the box of
// control limits in every direction
M3_PC_HD float prior_controller_speed(float factor, float u_max0, float u_max1) {
    return factor * fminf(fabsf(u_max0), fabsf(u_max1));
}

// |(x, y)|: two products, one sum, one root
M3_PC_HD float prior_controller_norm(float x, float y) { return sqrtf(x * x + y * y); }

// ONE step of a saturated proportional drive from (px, py) toward (tx, ty): the step covers what is left of the way, at most
// speed * dt of it.  Leaves the control in (ux, uy) and moves (px, py).
M3_PC_HD void prior_controller_drive(float& px, float& py, float tx, float ty, float dt, float speed, float& ux, float& uy) {
    const float dx = tx - px, dy = ty - py;
    const float dist = prior_controller_norm(dx, dy);
    ux = 0.0f; uy = 0.0f;
    if (dist > 0.0f) {
        const float v = fminf(dist / dt, speed);
        ux = (dx / dist) * v;
        uy = (dy / dist) * v;
    }
    px = px + ux * dt;
    py = py + uy * dt;
}

// the point `standoff` behind the box on the goal-box line (a box at the goal: behind it along +x)
M3_PC_HD void prior_controller_behind(float bx, float by, float gx, float gy, float standoff, float& hx, float& hy) {
    float ax = bx - gx, ay = by - gy;
    const float len = prior_controller_norm(ax, ay);
    if (len > 0.0f) { ax = ax / len; ay = ay / len; }
    else { ax = 1.0f; ay = 0.0f; }
    hx = bx + standoff * ax;
    hy = by + standoff * ay;
}

// One sequence of T controls; emit(t, ux, uy) receives step t's.
// GO_TO: T drive steps from the robot (rx, ry) toward the goal (gx, gy); (bx, by), standoff and reach are not read.
// PUSH_BEHIND: toward the point behind the box until the robot is within `reach` of it (tested before each step), toward the
// goal from then on.
template <class Emit>
M3_PC_HD void prior_controller_sequence(int kind, float rx, float ry, float bx, float by, float gx, float gy, int T, float dt,
                                        float speed, float standoff, float reach, Emit emit) {
    float px = rx, py = ry, tx = gx, ty = gy, hx = gx, hy = gy;
    bool switched = kind != PRIOR_CONTROLLER_PUSH_BEHIND;
    if (!switched) prior_controller_behind(bx, by, gx, gy, standoff, hx, hy);
    for (int t = 0; t < T; ++t) {
        if (!switched && prior_controller_norm(hx - px, hy - py) <= reach) switched = true;
        tx = switched ? gx : hx;
        ty = switched ? gy : hy;
        float ux, uy;
        prior_controller_drive(px, py, tx, ty, dt, speed, ux, uy);
        emit(t, ux, uy);
    }
}

}  // namespace m3
